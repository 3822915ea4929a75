// bwt_headbits_check.cc — the grouping of a round >= 2 as one head byte per slot (ghead[]: what bwt_apply leaves for the tile sorters
// and bwt_gather_keys), against the serial model of bwt_rules_check.cc (an array of slots cut into numbered groups) over the same
// random group-size sequences (the same generator and seed).  Every window is walked the way ts_window does it: the mask words from
// the head bytes, 16 to a thread through hf_bits4; the look-back over the TS_MAXGRP head bytes in front of the window, four to a
// thread through ts_li4 on head bits; ts_prev_end from both.  Checked: the mask words are the model's heads; prev_end is the
// model's; wherever the window's first slot is no head the look-back on head bits gives ts_prev_end the same number as the
// look-back on ordinals; the ordinals that bwt_gather_keys counts out of the head bytes are the model's; and the deferred groups,
// numbered from the head bits of their slots alone, come out dense and in order.
// Stand-alone: built with the host compiler under the address / undefined-behaviour sanitizers and run by
// tests/test_bwt_headbits_host.py.  Exit 0 = all checks passed; a failing check prints itself and the program exits 1.
#include "bwt_rules.h"
#include <stdio.h>
#include <string.h>
#include <vector>

using namespace cjs;

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_fail < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } g_fail++; } } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }

struct Groups {
  std::vector<uint32_t> start, size;      // per group
  std::vector<uint32_t> gord;             // per slot: the ordinal of its group
  std::vector<uint8_t> ghead;             // per slot: 1 = starts a group (padded to a multiple of 16 with bytes that must not count)
  uint32_t A = 0;
  void add(uint32_t m) {
    start.push_back(A); size.push_back(m); gord.insert(gord.end(), m, (uint32_t)start.size() - 1u);
    ghead.push_back(1); ghead.insert(ghead.end(), m - 1, 0); A += m;
  }
  void pad() { while (ghead.size() % 16) ghead.push_back(0xFF); }
};
static const uint32_t kSizes[] = {2, 3, 63, 64, 65, 1023, 1024, 1025, 3071, 3072, 3073, 5000};
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
        if (rnd() & 1) m = m > 700 ? 1 + (uint32_t)(rnd() % 700) : m;
      }
    }
    if (m == 0) m = 1;
    g.add(m < left ? m : left);
  }
  g.pad();
  return g;
}
static uint32_t word_at(const std::vector<uint8_t>& b, uint64_t at) { uint32_t w; memcpy(&w, &b[at], 4); return w; }      // (little-endian, as the device)

static void check_windows(const Groups& g, int seq) {
  const uint32_t A = g.A, nwin = ts_windows(A);
  for (uint32_t win = 0; win < nwin; win++) {
    const uint64_t wb = ts_win_base(win);
    const uint32_t L = ts_win_len(wb, A);
    const bool at_end = wb + L == A;
    // thread t: the head bytes of slots [16t, 16t + 16) of the window, those below L, as 16 bits of the mask words
    uint64_t hm[64] = {0};
    for (uint32_t t = 0; t < 256; t++) {
      const uint32_t first = 16 * t, nv = L > first ? (L - first < 16 ? L - first : 16) : 0;
      if (!nv) continue;
      uint32_t m16 = 0;
      for (int q = 0; q < 4; q++) m16 |= hf_bits4(word_at(g.ghead, wb + first + 4 * q), 0) << (4 * q);
      hm[t >> 2] |= (uint64_t)(m16 & ((1u << nv) - 1u)) << (16 * (t & 3));
    }
    for (uint32_t x = 0; x < TS_WIN; x++) {
      const bool want = x < L && (wb + x == 0 || g.gord[wb + x] != g.gord[wb + x - 1]);
      CHECK((((hm[x >> 6] >> (x & 63)) & 1ull) != 0) == want, "seq %d window %u slot %u: head bit %d", seq, win, x, (int)!want);
    }
    int wnext[64];
    for (int i = 63, next = TS_NO_NEXT; i >= 0; i--) { wnext[i] = next; if (hm[i]) next = word_first(hm[i], i); }
    uint32_t li_bits = 0, li_ord = 0;
    if (wb) for (uint32_t t = 0; t < TS_MAXGRP / 4; t++) {
      const uint64_t at = wb - TS_MAXGRP + 4 * t;
      const uint32_t lb = ts_li4(t, hf_bits4(word_at(g.ghead, at), 0));
      const uint32_t* q = &g.gord[at];
      const uint32_t lo = ts_li4(t, q[0], q[1], q[2], q[3], g.gord[wb]);
      if (lb > li_bits) li_bits = lb;
      if (lo > li_ord) li_ord = lo;
    }
    const uint32_t prev_end = ts_prev_end(wb, L, at_end, li_bits, hm[0], wnext[0]);
    const uint32_t g0 = g.gord[wb];
    const uint32_t want_prev = g.start[g0] < wb && g.size[g0] <= TS_MAXGRP ? (uint32_t)(g.start[g0] + g.size[g0] - wb) : 0u;
    CHECK(prev_end == want_prev, "seq %d window %u: prev_end %u from head bits, the model says %u", seq, win, prev_end, want_prev);
    CHECK(prev_end == ts_prev_end(wb, L, at_end, li_ord, hm[0], wnext[0]), "seq %d window %u: prev_end from head bits and from ordinals differ", seq, win);
    if (wb && !(hm[0] & 1ull)) {
      CHECK(li_bits == li_ord, "seq %d window %u: look-back %u on head bits, %u on ordinals", seq, win, li_bits, li_ord);
      CHECK(li_bits == (g.start[g0] + TS_MAXGRP > wb ? (uint32_t)(g.start[g0] + TS_MAXGRP - wb) : 0u), "seq %d window %u: look-back %u, the group starts at %u", seq, win, li_bits, g.start[g0]);
    }
  }
}

// ordinals out of the head bytes (bwt_gather_keys): heads up to and including the slot, less one; and the deferred groups (the
// groups of more than TS_MAXGRP slots: no window owns them) numbered from the head bits of the deferred slots alone
static void check_ordinals(const Groups& g, int seq) {
  uint32_t heads = 0, dheads = 0, dgroups = 0;
  std::vector<uint32_t> dpre(g.size.size());      // the model: deferred groups up to and including group gi
  for (uint32_t gi = 0; gi < g.size.size(); gi++) { dgroups += g.size[gi] > TS_MAXGRP; dpre[gi] = dgroups; }
  for (uint32_t a = 0; a < g.A; a++) {
    const uint32_t bit = g.ghead[a] & 1u;
    heads += bit;
    CHECK(heads - 1u == g.gord[a], "seq %d slot %u: ordinal %u out of the head bytes, the model says %u", seq, a, heads - 1u, g.gord[a]);
    const bool deferred = g.size[g.gord[a]] > TS_MAXGRP;
    const uint64_t key = round_key(bit, RANK_MASK);      // what the tile sorters leave for a slot they do not own
    if (deferred) {
      dheads += (uint32_t)(round_key_ordinal(key) & 1ull);
      const uint32_t want = dpre[g.gord[a]];
      CHECK(dheads == want && round_key_rank(key) == RANK_MASK, "seq %d slot %u: deferred group %u, the model says %u", seq, a, dheads, want);
    }
  }
  CHECK(dheads == dgroups && heads == g.size.size(), "seq %d: %u deferred groups of %u, %u groups of %zu", seq, dheads, dgroups, heads, g.size.size());
}

int main() {
  const uint32_t ends[] = {0, 1, 2, 63, 64, 1023, 1024, 1025, 2000, 3071};
  for (int seq = 0; seq < 3000; seq++) {
    const uint32_t total = (uint32_t)(rnd() % 12) * TS_NOM + (seq % 3 ? ends[rnd() % 10] : (uint32_t)(rnd() % TS_NOM));
    const Groups g = random_groups(total ? total : 1);
    check_windows(g, seq);
    check_ordinals(g, seq);
  }
  // a group that starts d slots in front of a window, every d around the ends of the look-back, and the window's first slot a head
  for (uint32_t d : {0u, 1u, 2u, 3u, 4u, 5u, 63u, 64u, 65u, 1020u, 1021u, 1022u, 1023u, 1024u, 1025u}) for (uint32_t m : {2u, 64u, 1023u, 1024u, 1025u, 1100u}) {
    Groups g; g.add(TS_NOM - d - 7); g.add(7); if (d) g.add(d < m ? m : d); else g.add(m); g.add(m); g.add(TS_NOM); g.pad();
    check_windows(g, 100000 + (int)d);
    check_ordinals(g, 100000 + (int)d);
  }
  for (uint32_t t = 0; t < 256; t++) for (uint32_t h = 0; h < 16; h++) {
    uint32_t want = 0;
    for (uint32_t j = 0; j < 4; j++) if ((h >> j) & 1u) want = 4 * t + j;
    CHECK(ts_li4(t, h) == want, "ts_li4(%u, %x) = %u, want %u", t, h, ts_li4(t, h), want);
  }
  if (g_fail) { printf("bwt_headbits_check: %d checks FAILED\n", g_fail); return 1; }
  printf("bwt_headbits_check ok\n");
  return 0;
}
