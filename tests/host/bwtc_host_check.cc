// bwtc_host_check.cc — the host side of BWTC (csrc/bwtc_host.h: range coder, its two-thread split, framing, batch plan;
// csrc/bwtc_decode.h: the entropy decoder of untrusted streams; csrc/bwtc_format.h) against the oracle, without a GPU.
// Stand-alone: built with the host compiler, once under the address / undefined-behaviour sanitizers and once under the thread
// sanitizer, and run by tests/test_bwtc_host_check.py, which passes the crafted step lists of tests/bwtc_cases.py as argv[1]
// (per list two 64-bit words, first byte and step count, then the steps).  Exit 0 = all checks passed; a failing check prints
// itself and the program exits 1.
#include "bwtc_host.h"
#include "bwtc_decode.h"
#include "cjs_oracle.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <map>
#include <string>
#include <vector>

using namespace cjs;
typedef std::vector<uint8_t> Bytes;

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_fail < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } g_fail++; } } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }

static Bytes take(uint8_t* p, size_t n) { Bytes v(p, p + n); cjs_oracle_free(p); return v; }

// encodeStart(first_byte, 1), the steps, encodeFinish, as cjs_stage_bwtc_code runs them
static Bytes run_coder(const uint64_t* steps, size_t n, int first_byte, bool split) {
  Bytes o;
  HostCoder coder(o);
  coder.start(first_byte, 1);
  if (split) coder.start_split();
  coder.reserve_steps(n);
  code_steps(coder, steps, (uint32_t)n, rcp_table());
  coder.reserve_steps(64);
  coder.finish();
  CHECK(!coder.failed.load(), "the low thread ran out of memory");
  return o;
}
static void coder_equals_oracle(const char* what, const std::vector<uint64_t>& steps, int first_byte) {
  uint8_t* w = nullptr; size_t wn = 0;
  for (uint64_t st : steps) if (!step_valid(st)) { CHECK(false, "%s: invalid step %llx", what, (unsigned long long)st); return; }
  const int rc = cjs_oracle_rc_encode_steps(first_byte, steps.data(), steps.size(), &w, &wn, nullptr);
  CHECK(rc == 0, "%s: oracle coder rc %d", what, rc);
  if (rc) return;
  const Bytes want = take(w, wn);
  for (int split = 0; split < 2; split++) {
    const Bytes got = run_coder(steps.data(), steps.size(), first_byte, split != 0);
    CHECK(got == want, "%s (%s, %zu steps): %zu bytes, oracle %zu", what, split ? "split" : "one thread", steps.size(), got.size(), want.size());
  }
}

// (a) the crafted step lists
static void coder_cases(const char* path) {
  FILE* f = fopen(path, "rb");
  CHECK(f != nullptr, "cannot open %s", path);
  if (!f) return;
  uint64_t head[2]; int ncase = 0;
  while (fread(head, 8, 2, f) == 2) {
    std::vector<uint64_t> steps(head[1]);
    if (head[1] && fread(steps.data(), 8, steps.size(), f) != steps.size()) { CHECK(false, "short step list %d", ncase); break; }
    char what[32]; snprintf(what, sizeof what, "list %d", ncase++);
    coder_equals_oracle(what, steps, (int)head[0]);
  }
  fclose(f);
  CHECK(ncase > 0, "no step lists in %s", path);
}

// (b) more steps than the ring holds: the ring wraps and the range side finds it full
static void ring_wrap() {
  Bytes in(400000);
  for (auto& b : in) b = (uint8_t)(rnd() >> 32);
  uint64_t* steps = nullptr; size_t ns = 0, prefix = 0; int fb = 0; uint64_t lo[4], hi[4];
  const long nb = cjs_oracle_bwtc_stream_steps(in.data(), in.size(), 9, &steps, &ns, &prefix, &fb, lo, hi, 4);
  CHECK(nb == 1, "stream steps: %ld blocks", nb);
  if (nb < 0) return;
  CHECK(ns > (size_t)HostCoder::RING * HostCoder::RCAP, "%zu steps do not fill the ring of %u", ns, HostCoder::RING * HostCoder::RCAP);
  const std::vector<uint64_t> v(steps, steps + ns);
  cjs_oracle_free(steps);
  coder_equals_oracle("ring wrap", v, fb);
}

// one input at one level with what the oracle makes of it: the stream, every coder step of it with the blocks' model sections
// [lo, hi), and per block the sentinel-BWT column and primary index
struct Case {
  std::string name; Bytes in; int level;
  Bytes stream;
  std::vector<uint64_t> steps, lo, hi; size_t prefix = 0; int first_byte = 0;
  Bytes cols; std::vector<uint32_t> lens, pidx;
};
static bool ask_oracle(Case& c) {
  const uint32_t bs = (uint32_t)c.level * 100000u;
  uint8_t* w = nullptr; size_t wn = 0;
  int rc = cjs_oracle_bwtc_compress(c.in.data(), c.in.size(), c.level, &w, &wn);
  CHECK(rc == 0, "%s: oracle compress rc %d", c.name.c_str(), rc);
  if (rc) return false;
  c.stream = take(w, wn);
  const long cap = (long)(c.in.size() / bs) + 2;
  c.lo.resize(cap); c.hi.resize(cap);
  uint64_t* steps = nullptr; size_t ns = 0;
  const long nb = cjs_oracle_bwtc_stream_steps(c.in.data(), c.in.size(), c.level, &steps, &ns, &c.prefix, &c.first_byte, c.lo.data(), c.hi.data(), cap);
  CHECK(nb >= 0 && nb < cap, "%s: stream steps %ld", c.name.c_str(), nb);
  if (nb < 0) return false;
  c.steps.assign(steps, steps + ns);
  cjs_oracle_free(steps);
  Bytes U(bs);
  for (size_t at = 0; at < c.in.size(); at += bs) {
    const uint32_t length = (uint32_t)std::min<size_t>(bs, c.in.size() - at);
    const int pidx = cjs_oracle_bwt_sentinel(c.in.data() + at, (int)length, U.data());
    CHECK(pidx >= 0, "%s: oracle BWT", c.name.c_str());
    c.pidx.push_back((uint32_t)pidx); c.lens.push_back(length);
    c.cols.insert(c.cols.end(), U.begin(), U.begin() + length);
  }
  CHECK((long)c.lens.size() == nb, "%s: %ld blocks of steps, %zu of input", c.name.c_str(), nb, c.lens.size());
  return (long)c.lens.size() == nb;
}

// (c) the compressor's host path with the oracle standing in for the GPU stages: stream head, per block its head and its model
// steps, "no more blocks", finish
static Bytes host_encode(const Case& c, bool split) {
  const uint32_t bs = (uint32_t)c.level * 100000u;
  const size_t nb = c.lens.size();
  Bytes o;
  const int first = write_stream_head(o, c.in.size(), false);
  CHECK(first == c.first_byte && o.size() == c.prefix, "%s: head %d / %zu bytes, oracle %d / %zu", c.name.c_str(), first, o.size(), c.first_byte, c.prefix);
  HostCoder coder(o);
  coder.start(first, 1);
  if (split && nb) coder.start_split();
  coder.shift(1, (uint32_t)c.level, 8);
  for (size_t k = 0; k < nb; k++) {
    const uint8_t* blk = c.in.data() + k * bs;
    bool used[256] = {false}; uint8_t alist[256]; uint32_t asz = 0;         // the alphabet: the bytes present in the block
    for (uint32_t i = 0; i < c.lens[k]; i++) used[blk[i]] = true;
    for (int b = 0; b < 256; b++) if (used[b]) alist[asz++] = (uint8_t)b;
    coder.reserve_steps((size_t)(c.hi[k] - c.lo[k]));
    code_block_head(coder, bs, c.lens[k], c.pidx[k], alist, asz);
    code_steps(coder, c.steps.data() + c.lo[k], (uint32_t)(c.hi[k] - c.lo[k]), rcp_table());
  }
  coder.reserve_steps(64);
  coder.freq(1, 2, 3);
  coder.finish();
  CHECK(!coder.failed.load(), "the low thread ran out of memory");
  return o;
}

// (d) the decoder gives the oracle's sentinel-BWT columns and primary indices
static void decode_equals_oracle(const Case& c) {
  BwtcBlocks B;
  const int rc = bwtc_entropy_decode(c.stream.data(), c.stream.size(), B, false);
  CHECK(rc == 0 && B.level == c.level, "%s: decode rc %d level %d", c.name.c_str(), rc, B.level);
  CHECK(B.lens == c.lens && B.pidx == c.pidx && B.cols == c.cols, "%s: %zu blocks / %zu bytes decoded, oracle %zu / %zu", c.name.c_str(), B.lens.size(), B.cols.size(), c.lens.size(), c.cols.size());
}
// damaged streams: any return code will do, the sanitizers watch the call
static int g_decoded = 0;
static void must_return(const uint8_t* p, size_t n) {
  const Bytes copy(p, p + n);               // a heap block of exactly n bytes: a read past the end is seen
  BwtcBlocks B;
  const int rc = bwtc_entropy_decode(copy.data(), copy.size(), B, false);
  g_decoded += rc == 0;
}
static std::vector<Case> g_cases;      // of stream_cases, for decoder_fuzz
static void decoder_fuzz() {
#ifdef __SANITIZE_THREAD__
  printf("(one thread, thousands of calls: left to the address / undefined-behaviour build)\n");
  return;
#endif
  const Case* pick[2] = {nullptr, nullptr};            // the largest stream under 4 KiB of level 1 and of level 9
  for (const Case& c : g_cases) {
    const int w = c.level == 1 ? 0 : c.level == 9 ? 1 : -1;
    if (w >= 0 && c.stream.size() < 4096 && (!pick[w] || c.stream.size() > pick[w]->stream.size())) pick[w] = &c;
  }
  CHECK(pick[0] && pick[1] && pick[0]->stream.size() > 256 && pick[1]->stream.size() > 256, "no stream of 256..4095 bytes to damage");
  if (!pick[0] || !pick[1]) return;
  for (const Case* c : pick) for (size_t cut = 0; cut < c->stream.size(); cut++) must_return(c->stream.data(), cut);
  for (int it = 0; it < 2000; it++) {
    Bytes bad = pick[it & 1]->stream;
    bad[rnd() % bad.size()] ^= (uint8_t)(1u << (rnd() % 8));
    must_return(bad.data(), bad.size());
  }
  for (int it = 0; it < 200; it++) {
    Bytes junk = {'b', 'w', 't', 'c', 0x81};
    const size_t tail = it < 8 ? (size_t)it + 1 : 1 + rnd() % 5000;
    for (size_t i = 0; i < tail; i++) junk.push_back((uint8_t)(rnd() >> 24));
    must_return(junk.data(), junk.size());
  }
}

static void stream_cases() {
  std::vector<std::pair<std::string, Bytes>> inputs;
  inputs.push_back({"empty", Bytes()});
  inputs.push_back({"one byte", Bytes(1, 'x')});
  inputs.push_back({"banana", Bytes({'b', 'a', 'n', 'a', 'n', 'a'})});
  for (size_t n : {100000u, 100001u}) {                  // at level 1: an exact block, and one byte over it
    Bytes v(n);
    for (auto& b : v) b = (uint8_t)("etaoin shrdlu"[rnd() % 13] ^ (rnd() % 11 == 0 ? 0x20 : 0));
    inputs.push_back({n == 100000u ? "100000 text-like" : "100001 text-like", v});
  }
  inputs.push_back({"120000 zeros", Bytes(120000, 0)});
  Bytes skew(70000);
  for (auto& b : skew) b = rnd() % 64 ? 'e' : (uint8_t)(rnd() >> 40);
  inputs.push_back({"70000 skewed", skew});
  for (const auto& in : inputs) for (int level : {1, 5, 9}) {
    Case c;
    c.name = in.first + " level " + std::to_string(level); c.in = in.second; c.level = level;
    if (!ask_oracle(c)) continue;
    for (int split = 0; split < 2; split++) {
      const Bytes got = host_encode(c, split != 0);
      CHECK(got == c.stream, "%s (%s): %zu bytes, oracle %zu", c.name.c_str(), split ? "split" : "one thread", got.size(), c.stream.size());
    }
    decode_equals_oracle(c);
    g_cases.push_back(c);
  }
}

// (e) the batch plan by property
static void plan_cases() {
  for (uint32_t nb : {1u, 2u, 7u, 8u, 16u, 17u, 513u, 1025u}) for (uint32_t slots : {1u, 2u, 3u, 64u}) for (uint32_t fb : {0u, 1u, 8u}) {
    const int ndev = 3, dev0 = 2;
    const uint32_t nslots = plan_slots(slots, nb);
    CHECK(nslots >= 1 && nslots <= slots && nslots <= nb, "nb %u slots %u: %u slots", nb, slots, nslots);
    const std::vector<BatchPlan> plan = plan_batches(nb, nslots, ndev, dev0, fb);
    std::map<int, std::vector<BatchPlan>> by_slot;
    uint32_t next = 0; int last_slot = -1;
    for (const BatchPlan& b : plan) {
      CHECK(b.first == next && b.count >= 1 && b.count <= BWTC_MAX_BATCH, "nb %u slots %u fb %u: batch [%u, +%u) behind %u", nb, slots, fb, b.first, b.count, next);      // a partition of [0, nb) in order
      CHECK(b.slot >= last_slot && b.slot < (int)nslots, "nb %u slots %u fb %u: slot %d behind %d", nb, slots, fb, b.slot, last_slot);             // one contiguous range per slot
      CHECK(b.seq == (int)by_slot[b.slot].size(), "nb %u slots %u fb %u: seq %d of slot %d", nb, slots, fb, b.seq, b.slot);
      CHECK(b.device == (nslots == 1 ? dev0 : b.slot % ndev), "nb %u slots %u fb %u: slot %d on device %d", nb, slots, fb, b.slot, b.device);
      next = b.first + b.count; last_slot = b.slot;
      by_slot[b.slot].push_back(b);
    }
    CHECK(next == nb, "nb %u slots %u fb %u: batches end at %u", nb, slots, fb, next);
    for (const auto& sv : by_slot) {
      const std::vector<BatchPlan>& v = sv.second;
      const uint32_t range = v.back().first + v.back().count - v.front().first;
      const bool small_first = sv.first == 0 && fb && range > 2 * fb;       // the first-batch rule: slot 0, seq 0, enough blocks behind it
      for (size_t i = 0; i < v.size(); i++) {
        if (i == 0 && small_first) CHECK(v[i].count == fb, "nb %u slots %u fb %u: first batch of %u", nb, slots, fb, v[i].count);
        else if (i + 1 < v.size()) CHECK(v[i].count == BWTC_MAX_BATCH, "nb %u slots %u fb %u: batch %zu of slot %d holds %u", nb, slots, fb, i, sv.first, v[i].count);
      }
      if (!small_first) CHECK(v.size() == (range + BWTC_MAX_BATCH - 1) / BWTC_MAX_BATCH, "nb %u slots %u fb %u: slot %d in %zu batches", nb, slots, fb, sv.first, v.size());
    }
  }
}

int main(int argc, char** argv) {
  if (argc < 2) { printf("usage: bwtc_host_check <step lists>\n"); return 2; }
  struct { const char* name; void (*run)(); } parts[] = {{"ring wrap", ring_wrap}, {"streams", stream_cases}, {"damaged streams", decoder_fuzz}, {"batch plan", plan_cases}};
  clock_t t = clock();
  coder_cases(argv[1]);
  printf("step lists: %.1f s of cpu\n", (double)(clock() - t) / CLOCKS_PER_SEC);
  for (auto& p : parts) { t = clock(); p.run(); printf("%s: %.1f s of cpu\n", p.name, (double)(clock() - t) / CLOCKS_PER_SEC); }
  if (g_fail) { printf("%d check(s) failed\n", g_fail); return 1; }
  printf("%d damaged streams decoded to something\nbwtc_host_check ok\n", g_decoded);
  return 0;
}
