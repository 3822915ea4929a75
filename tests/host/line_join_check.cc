// line_join_check.cc -- csrc/line_join.h on the CPU (tests/test_line_join_host_check.py builds this with the host compiler under the
// address and undefined-behaviour sanitizers and runs it; no HIP, nothing loaded into Python).
//   LkJoin over random texts of a small alphabet cut into random blocks (empty ones, ones without a newline, lines over three and
//   more blocks), the blocks' records, tails and head_h2 made here from lk_push / lk_key, fed in batches of random size: random
//   windows and caps, both destinations, bad blocks and both tail rules, against lk_text_keys of the whole text
//   text_keys_work_bytes against the layout of the pieces and tiles a text really has
#include "line_join.h"
#include "scan_plan.h"
#include <stdio.h>
#include <set>
#include <string>
#include <vector>

using namespace cjs;

static int fails = 0;
#define CHECK(cond) do { if (!(cond)) { if (fails++ < 20) fprintf(stderr, "%s:%d (text %d): %s\n", __FILE__, __LINE__, g_text, #cond); } } while (0)
static int g_text = -1;

static uint64_t rng_state = 0x13198A2E03707344ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

static bool same(const cjs_bz_linekey& a, const cjs_bz_linekey& b) { return a.hash == b.hash && a.len == b.len && a.check == b.check; }
static const cjs_bz_linekey GUARD{0x5EA1ED5EA1ED5EA1ull, 0x5EA1EDu, 0xC0FFEEu};

// What the kernels give the host for one block: a record per newline, the fragment behind the last, H_B2 of the first record in full.
struct Block { std::vector<cjs_bz_linekey> recs; LkTail tail; };
static Block block_of_bytes(const std::string& s, const LkBases& B) {
  Block k;
  k.tail = LkTail{0, 0, 0, 0, 0};
  LkFrag f{0, 0, 0};
  for (unsigned char c : s) {
    lk_push(f, B, c);
    if (c != 0x0A) continue;
    if (k.recs.empty()) k.tail.head_h2 = f.h2;
    k.recs.push_back(lk_key(f));
    f = LkFrag{0, 0, 0};
  }
  k.tail.h1 = f.h1; k.tail.h2 = f.h2; k.tail.len = (uint32_t)f.len;
  return k;
}

struct Case {
  std::string text;
  std::vector<uint64_t> off;                                // the blocks
  cjs_bz_lines t;
  std::vector<Block> blk;
  std::vector<cjs_bz_linekey> whole;                        // lk_text_keys of the text: N + 1 of them
  std::vector<uint32_t> nl_block;                           // the block of newline j + 1
  LkBases B;
  uint64_t seed;
};

static Case random_case(int it) {
  Case c;
  c.seed = rnd();
  c.B = lk_bases(c.seed);
  const size_t n = it % 25 == 0 ? 0 : (size_t)(rnd() % (it % 5 == 0 ? 40 : 400));
  const int nl_one_in = it % 6 == 0 ? 0 : 2 + (int)(rnd() % (it % 4 == 0 ? 60 : 8));      // (0: no newline at all)
  for (size_t i = 0; i < n; i++) c.text.push_back(nl_one_in && rnd() % (uint64_t)nl_one_in == 0 ? '\n' : (char)('a' + rnd() % 2));
  if (n && it % 3 == 0) c.text.back() = '\n';
  if (n && it % 3 == 1) c.text.back() = 'a';
  // blocks: short ones when lines are long (a line over three blocks and more), about one in five empty, empty ones at both ends
  const uint64_t max_size = it % 4 == 0 ? 3 : 1 + rnd() % 60;
  c.off.assign(1, 0);
  if (it % 7 == 0) c.off.push_back(0);
  while (c.off.back() < n) c.off.push_back(rnd() % 5 == 0 ? c.off.back() : std::min<uint64_t>(n, c.off.back() + 1 + rnd() % max_size));
  if (it % 7 == 1 || c.off.size() == 1) c.off.push_back(c.off.back());
  c.t.cum.assign(1, 0);
  c.t.total_bytes = n;
  for (size_t b = 0; b + 1 < c.off.size(); b++) {
    c.blk.push_back(block_of_bytes(c.text.substr((size_t)c.off[b], (size_t)(c.off[b + 1] - c.off[b])), c.B));
    c.t.nl.push_back((uint32_t)c.blk.back().recs.size());
    c.t.cum.push_back(c.t.cum.back() + c.blk.back().recs.size());
    for (size_t j = 0; j < c.blk.back().recs.size(); j++) c.nl_block.push_back((uint32_t)b);
  }
  c.whole.assign((size_t)c.t.cum.back() + 1, GUARD);
  const size_t lines = lk_text_keys((const uint8_t*)c.text.data(), n, c.seed, c.whole.data(), c.whole.size());
  CHECK(lines == c.whole.size());
  return c;
}

// One run of the join over the touched blocks, the bad ones left out, in batches of random size.  Host destination: into keys
// (cap).  Device destination (dev != nullptr): the whole-line records go to dev as LineKeysCall::batch copies them, the join sees a
// block's first record alone; the fills and the patches are applied at the end.
struct Ran { size_t patches = 0; bool tail_dropped = false; };
static Ran run_join(const Case& c, uint64_t first, uint64_t end, const std::vector<uint32_t>& touched, const std::set<uint32_t>& bad, cjs_bz_linekey* keys,
                    size_t cap, cjs_bz_linekey* dev, bool tally_tail) {
  LkJoin J;
  J.t = &c.t; J.B = c.B; J.first = first; J.end = end; J.keys = keys; J.cap = cap; J.touched = &touched; J.d_keys = dev; J.tally_tail = tally_tail;
  for (size_t g0 = 0; g0 < touched.size();) {
    const size_t g1 = std::min(touched.size(), g0 + 1 + (size_t)(rnd() % 4));
    std::vector<cjs_bz_linekey> recs; std::vector<uint32_t> which; std::vector<size_t> rec0;      // the batch's good blocks, their records packed
    for (size_t k = g0; k < g1; k++) {
      const uint32_t b = touched[k];
      if (bad.count(b)) continue;
      which.push_back(b); rec0.push_back(recs.size());
      recs.insert(recs.end(), c.blk[b].recs.begin(), c.blk[b].recs.end());
    }
    recs.push_back(GUARD);                                   // (a block without a record: a valid pointer all the same)
    for (size_t i = 0; i < which.size(); i++) {
      const uint32_t b = which[i];
      const size_t nrec = c.blk[b].recs.size();
      if (dev) {
        const uint64_t l0 = c.t.cum[b], lo = std::max<uint64_t>(l0, first), hi = std::min<uint64_t>(l0 + nrec, end);
        for (uint64_t q = lo; q < hi; q++) dev[q - first] = recs[rec0[i] + (size_t)(q - l0)];
        const cjs_bz_linekey head = nrec ? recs[rec0[i]] : cjs_bz_linekey{0, 0, 0};      // lk_heads
        J.good(b, &head, c.blk[b].tail);
      } else J.good(b, recs.data() + rec0[i], c.blk[b].tail);
    }
    g0 = g1;
  }
  J.finish();
  Ran r;
  r.tail_dropped = J.tail_dropped;
  if (!dev) { CHECK(J.patches.empty() && J.fills.empty() && !J.tail_dropped); return r; }
  r.patches = J.patches.size();
  CHECK(J.patches.size() <= touched.size() + 1);
  for (const auto& f : J.fills) {
    CHECK(f.first < f.second && f.second <= end - first);
    for (uint64_t i = f.first; i < f.second && i < end - first; i++) dev[i] = lk_bad_key();
  }
  std::set<uint64_t> at;
  for (const LkPatch& p : J.patches) {
    CHECK(at.insert(p.at).second);                           // no `at` twice
    CHECK(p.at < end - first);
    if (p.at < end - first) dev[p.at] = p.key;
  }
  return r;
}

static void check_case(const Case& c) {
  const uint64_t N = c.t.cum.back();
  const size_t nb = c.off.size() - 1;
  for (int w = 0; w < 8; w++) {
    const uint64_t first = w == 0 ? 0 : rnd() % (N + 1);
    const uint64_t end = w < 3 ? N + 1 : line_window_end(first, 1 + rnd() % (N + 2), N);
    const uint64_t nwin = end - first;
    const std::vector<uint32_t> touched = line_window_blocks(c.t.cum, c.t.total_bytes, c.off, first, end);
    std::set<uint32_t> bad;
    if (w % 2) for (uint32_t b : touched) if (rnd() % 3 == 0) bad.insert(b);
    // what every line of the window has to carry: its key, or the bad key if a bad block lies between the block of the newline
    // in front of it (whose bytes behind that newline are its start) and the block of its own newline (the tail: the last block)
    std::vector<cjs_bz_linekey> want((size_t)nwin);
    for (uint64_t q = first; q < end; q++) {
      const size_t b0 = q ? c.nl_block[(size_t)q - 1] : 0, b1 = q < N ? c.nl_block[(size_t)q] : nb - 1;
      bool is_bad = false;
      for (uint32_t b : bad) is_bad = is_bad || (b >= b0 && b <= b1);
      want[(size_t)(q - first)] = is_bad ? lk_bad_key() : c.whole[(size_t)q];
    }
    // (a), (c): the host destination under a random cap, guard words either side
    const size_t cap = w % 4 == 0 ? (size_t)nwin : (size_t)(rnd() % (nwin + 3)), room = (size_t)std::min<uint64_t>(cap, nwin);
    std::vector<cjs_bz_linekey> host(room + 2, GUARD);
    run_join(c, first, end, touched, bad, host.data() + 1, cap, nullptr, true);
    CHECK(same(host[0], GUARD) && same(host[room + 1], GUARD));
    for (size_t i = 0; i < room; i++) CHECK(same(host[1 + i], want[i]));
    // (b), (d) the plain tail rule: the device destination gives what the host destination gives
    std::vector<cjs_bz_linekey> dev((size_t)nwin + 2, GUARD);
    Ran r = run_join(c, first, end, touched, bad, nullptr, (size_t)nwin, dev.data() + 1, false);
    CHECK(same(dev[0], GUARD) && same(dev[(size_t)nwin + 1], GUARD) && !r.tail_dropped);
    for (size_t i = 0; i < nwin; i++) CHECK(same(dev[1 + i], want[i]));
    // (d) the tally's rule: the tail line, if the window holds it, is dropped when empty and keyed with a newline behind it otherwise
    std::fill(dev.begin(), dev.end(), GUARD);
    r = run_join(c, first, end, touched, bad, nullptr, (size_t)nwin, dev.data() + 1, true);
    CHECK(same(dev[0], GUARD) && same(dev[(size_t)nwin + 1], GUARD));
    const bool has_tail = end == N + 1;
    for (size_t i = 0; i + (has_tail ? 1 : 0) < nwin; i++) CHECK(same(dev[1 + i], want[i]));
    if (has_tail) {
      const size_t last_nl = c.text.rfind('\n');
      const std::string tail = c.text.substr(last_nl == std::string::npos ? 0 : last_nl + 1) + "\n";
      cjs_bz_linekey k;
      lk_text_keys((const uint8_t*)tail.data(), tail.size(), c.seed, &k, 1);
      const cjs_bz_linekey& got = dev[(size_t)nwin];
      if (lk_is_bad(want[(size_t)nwin - 1])) CHECK(lk_is_bad(got) && !r.tail_dropped);
      else if (tail.size() == 1) CHECK(r.tail_dropped && same(got, GUARD));
      else CHECK(!r.tail_dropped && same(got, k));
    } else CHECK(!r.tail_dropped);
  }
}

// text_keys_work_bytes is sized from upper bounds on the pieces and tiles of n bytes: never less than what text_keys_device carves
static void check_layout() {
  const size_t pieces[] = {1, 16383, 16384, 16385, 900000};
  for (size_t piece : pieces) {
    std::vector<size_t> ns = {0, 1, piece - 1, piece, piece + 1};
    for (size_t k = 1; k <= 3; k++) { ns.push_back(16384 * k - 1); ns.push_back(16384 * k + 1); }
    for (size_t n : ns) {
      const size_t np = text_keys_pieces(n, piece);
      size_t nt = 0;
      for (size_t i = 0; i < np; i++) nt += lk_tiles((uint32_t)std::min(piece, n - i * piece));
      CHECK(np * piece >= n && (np == 0 || (np - 1) * piece < n));
      CHECK(text_keys_work_bytes(n, piece) >= LkLayout(np, nt, 0, true).bytes + LkLayout::pad(sizeof(LkPatch) * (np + 1)));
    }
  }
  const LkLayout L(3, 5, 7, true), M(3, 5, 7, false);          // arrays in the order of the kernels' arguments, none overlapping
  CHECK(L.blk == 0 && L.cnt >= sizeof(LkBlk) * 3 && L.open >= L.cnt + 4 * 5 && L.tot >= L.open + sizeof(LkOpen) * 5 && L.tail >= L.tot + 4 * 3);
  CHECK(L.rec >= L.tail + sizeof(LkTail) * 3 && L.head >= L.rec + sizeof(cjs_bz_linekey) * 7 && L.bytes >= L.head + sizeof(cjs_bz_linekey) * 3 && M.bytes == M.head);
}

int main() {
  for (g_text = 0; g_text < 400; g_text++) check_case(random_case(g_text));
  g_text = -1;
  check_layout();
  if (fails) { fprintf(stderr, "%d checks failed\n", fails); return 1; }
  printf("line_join_check ok\n");
  return 0;
}
