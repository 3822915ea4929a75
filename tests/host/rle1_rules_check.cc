// rle1_rules_check.cc — the host-visible arithmetic of stage 0, csrc/rle1_rules.h (RLE1 chunking, block fill, share layout) and
// csrc/crc32_bz.h (CRC tables, GF(2) powers, address windows), checked by property against a byte-serial model of the reference's
// block reader and a bit-by-bit CRC, not by restating the formulas.
// Stand-alone: built with the host compiler under the address / undefined-behaviour sanitizers and run by
// tests/test_rle1_rules_host.py.  Exit 0 = all checks passed; a failing check prints itself and the program exits 1.
#include "crc32_bz.h"
#include "rle1_rules.h"
#include <stdio.h>
#include <string.h>
#include <vector>

using namespace cjs;

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_fail < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } g_fail++; } } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }
typedef unsigned long long ull;

// ---- the model: the block reader's run handling, byte by byte.  A run counter; the first four equal bytes go out as literals;
// the fourth reserves a count byte behind it, which every further equal byte increments; at 255 bytes the counter starts again.
struct Serial {
  int last = -1; uint32_t run = 0; uint64_t len = 0; uint64_t count_at = 0;
  uint64_t put(uint8_t c) {                      // returns the output position that takes the byte (its literal, or the count)
    if (c != last || run == 255) { last = c; run = 0; }
    run++;
    if (run <= 4) {
      const uint64_t at = len++;
      if (run == 4) count_at = len++;
      return at;
    }
    return count_at;
  }
};

static void check_chunk_rule() {
  Serial s;
  uint64_t sum = 0; uint32_t dp = 0;
  for (uint64_t m = 0; m <= 3000; m++) {
    CHECK(emitted_fresh(m) == s.len, "emitted_fresh(%llu) = %llu, the model has %llu", (ull)m, (ull)emitted_fresh(m), (ull)s.len);
    CHECK(emitted_fresh(m) == sum, "emitted_fresh(%llu) = %llu, chunk_emit along chunk_next sums to %llu", (ull)m, (ull)emitted_fresh(m), (ull)sum);
    const uint64_t at = s.put('a');                                   // byte d = m of the run
    CHECK(fresh_offset(m) == at, "fresh_offset(%llu) = %llu, the model puts the byte at %llu", (ull)m, (ull)fresh_offset(m), (ull)at);
    CHECK(dp == m % 255, "chunk_next reaches %u at byte %llu", dp, (ull)m);
    sum += chunk_emit(dp); dp = chunk_next(dp);
  }
}

// run_fill_input(cap) is the smallest m with emitted_fresh(m) >= cap: one pass of the model over a run long enough for the largest block
static void check_run_fill() {
  const uint32_t max_cap = 9 * 100000 - 19;
  std::vector<uint32_t> first_m(max_cap + 1, 0);
  Serial s;
  for (uint32_t m = 1; s.len < max_cap; m++) {
    const uint64_t before = s.len;
    s.put(0);
    for (uint64_t c = before + 1; c <= s.len && c <= max_cap; c++) first_m[c] = m;
  }
  auto one = [&](uint32_t cap) {
    const uint64_t m = run_fill_input(cap);
    CHECK(m == first_m[cap], "run_fill_input(%u) = %llu, the model fills the block at %u", cap, (ull)m, first_m[cap]);
    CHECK(emitted_fresh(m) >= cap && (m == 0 || emitted_fresh(m - 1) < cap), "emitted_fresh around run_fill_input(%u): %llu, %llu", cap, (ull)emitted_fresh(m - 1), (ull)emitted_fresh(m));
  };
  for (uint32_t cap = 1; cap <= 5000; cap++) one(cap);
  for (uint32_t level = 1; level <= 9; level++) one(level * 100000 - 19);
}

static void check_share_layout() {
  auto one = [&](uint32_t tpr) {
    const TileShare L = tile_share(tpr);
    const size_t off[6] = {L.lb, L.fb, L.gt, L.subpre, L.dmod, L.bytes};
    const size_t size[5] = {(size_t)8 * tpr, (size_t)8 * tpr, (size_t)8 * tpr, (size_t)32 * tpr, (size_t)16 * tpr};     // u64, u64, u64, u16[16], u8[16] per tile
    CHECK(off[0] == 0, "the share starts at %zu", off[0]);
    for (int i = 0; i < 5; i++) CHECK(off[i] + size[i] == off[i + 1], "tpr %u: section %d [%zu, +%zu) does not meet %zu", tpr, i, off[i], size[i], off[i + 1]);
    CHECK(L.lb % 8 == 0 && L.fb % 8 == 0 && L.gt % 8 == 0, "tpr %u: a u64 section is not 8-byte aligned", tpr);
    CHECK(L.subpre % 16 == 0 && L.dmod % 16 == 0 && L.bytes % 16 == 0, "tpr %u: a uint4-read section (or the next share) is not 16-byte aligned", tpr);
  };
  for (uint32_t tpr = 4; tpr <= 8192; tpr += 4) one(tpr);
  for (int i = 0; i < 3000; i++) {
    const uint64_t n = rnd() % (i % 3 ? (1ull << 22) : (1ull << 34));
    const uint32_t world = 1 + (uint32_t)(rnd() % 16), tpr = tiles_per_rank(n, world);
    CHECK(tpr % 4 == 0 && (uint64_t)tpr * world >= tiles_for(n), "tiles_per_rank(%llu, %u) = %u for %u tiles", (ull)n, world, tpr, tiles_for(n));
    CHECK((uint64_t)tiles_for(n) * RT >= n && (tiles_for(n) == 0 || (uint64_t)(tiles_for(n) - 1) * RT < n), "tiles_for(%llu) = %u", (ull)n, tiles_for(n));
    one(tpr);
  }
}

// ---- CRC: bit by bit, MSB first.  crc0 = zero initial value, no final inversion
static uint32_t crc0_bits(const uint8_t* p, size_t n, uint32_t reg = 0) {
  for (size_t i = 0; i < n; i++)
    for (int k = 7; k >= 0; k--) {
      const uint32_t top = (reg >> 31) ^ ((p[i] >> k) & 1u);
      reg = (reg << 1) ^ (top ? 0x04c11db7u : 0u);
    }
  return reg;
}
static uint32_t crc_bits(const uint8_t* p, size_t n) { return ~crc0_bits(p, n, 0xFFFFFFFFu); }
// x^(8n) mod P: below 2^32 as it stands; else the CRC0 of a one behind n - 4 zero bytes (CRC0(M) = M * x^32 mod P)
static uint32_t xpow8_bits(size_t n) {
  if (n < 4) return 1u << (8 * n);
  std::vector<uint8_t> m(n - 3, 0);
  m[0] = 1;
  return crc0_bits(m.data(), m.size());
}
// a * b mod P: carry-less product in 64 bits, then reduced from the top
static uint32_t mul_bits(uint32_t a, uint32_t b) {
  uint64_t prod = 0;
  for (int i = 0; i < 32; i++) if ((b >> i) & 1u) prod ^= (uint64_t)a << i;
  for (int i = 63; i >= 32; i--) if ((prod >> i) & 1u) prod ^= (0x100000000ull | 0x04c11db7u) << (i - 32);
  return (uint32_t)prod;
}

static const CrcTables g_tab = make_crc_tables();

static void check_crc_tables() {
  for (uint32_t i = 0; i < 256; i++)
    for (int k = 0; k < 4; k++) {
      const uint8_t m[4] = {(uint8_t)i, 0, 0, 0};
      CHECK(g_tab.tab[k][i] == crc0_bits(m, 1 + k), "tab[%d][%u]", k, i);
    }
  for (uint32_t r = 0; r < 64; r++) CHECK(g_tab.px[r] == xpow8_bits(r), "px[%u]", r);
  for (uint32_t q = 0; q < 256; q++) CHECK(g_tab.pw64[q] == xpow8_bits((size_t)64 * q), "pw64[%u]", q);
  for (int i = 0; i < 2000; i++) {
    const uint32_t a = (uint32_t)rnd(), b = (uint32_t)rnd();
    CHECK(gf_mul(a, b) == mul_bits(a, b), "gf_mul(%08x, %08x)", a, b);
  }
  for (int i = 0; i < 300; i++) {
    const size_t n = (size_t)(rnd() % (i < 200 ? 20000 : 200000));
    CHECK(gf_xpow8(n) == xpow8_bits(n), "gf_xpow8(%zu)", n);
    if (n < CRC_SEG) CHECK(gf_xpow8_small((uint32_t)n, g_tab.pw64, g_tab.px) == xpow8_bits(n), "gf_xpow8_small(%zu)", n);
  }
  const char* nine = "123456789";
  CHECK(crc_bits((const uint8_t*)nine, 9) == 0xFC891918u, "check value of the bit-by-bit CRC: %08x", crc_bits((const uint8_t*)nine, 9));
}

// the device's two steps on the host: a partial word per address window (64-byte pieces, each carried to the window's end), then
// the windows combined and the initial value carried through the whole range
static uint32_t crc_by_windows(const uint8_t* data, uint64_t S, uint64_t E, uint32_t* windows) {
  std::vector<uint32_t> seg;
  for (uint32_t i = 0; crc_window(S, E, i).W < E; i++) {
    const CrcWindow w = crc_window(S, E, i);
    CHECK(w.W % CRC_SEG == 0 && w.lo >= w.W && w.hi <= w.W + CRC_SEG && w.lo >= S && w.hi <= E && (i == 0 ? w.lo == S : w.lo == w.W),
          "window %u of [%llx, %llx): W %llx lo %llx hi %llx", i, (ull)S, (ull)E, (ull)w.W, (ull)w.lo, (ull)w.hi);
    uint32_t word = 0;
    for (uint32_t piece = 0; piece < CRC_SEG / 64; piece++) {
      const uint64_t ca = w.W + (uint64_t)piece * 64, cb = ca + 64;
      const uint64_t a = ca > w.lo ? ca : w.lo, b = cb < w.hi ? cb : w.hi;
      if (a >= b) continue;
      uint32_t crc = 0;
      for (uint64_t p = a; p < b; p++) crc = (crc << 8) ^ g_tab.tab[0][((crc >> 24) ^ data[p - S]) & 0xff];
      const uint32_t behind = (uint32_t)(w.hi - b);
      word ^= behind ? gf_mul(crc, gf_xpow8_small(behind, g_tab.pw64, g_tab.px)) : crc;
    }
    seg.push_back(word);
  }
  *windows = (uint32_t)seg.size();
  const uint32_t xfull = gf_mul(g_tab.pw64[255], g_tab.pw64[1]);
  uint32_t crc = 0, i = 0, covered = 0;
  for (; crc_window(S, E, i).W < E; i++) {
    const CrcWindow w = crc_window(S, E, i);
    const uint32_t l = (uint32_t)(w.hi - w.lo);
    covered += l;
    crc = gf_mul(crc, l == CRC_SEG ? xfull : gf_xpow8_small(l, g_tab.pw64, g_tab.px)) ^ seg[i];
  }
  CHECK(covered == E - S, "the windows of [%llx, %llx) hold %u bytes", (ull)S, (ull)E, covered);
  crc ^= gf_mul(0xFFFFFFFFu, gf_xpow8(E - S));
  return ~crc;
}

static void check_crc_windows() {
  std::vector<uint8_t> data(70000);
  const uint64_t base = 0x7f3a00000000ull;                             // a 16 KiB-aligned address
  for (int i = 0; i < 3000; i++) {
    const uint64_t off = i % 7 == 0 ? (i % 2 ? CRC_SEG - 1 : 0) : rnd() % CRC_SEG;
    uint64_t len = i % 5 == 0 ? rnd() % 70001 : rnd() % 3000;
    if (i % 11 == 0) len = (rnd() % 5) * CRC_SEG + rnd() % 3;          // whole windows, and one or two bytes more
    if (len > 70000) len = 70000;
    for (uint64_t k = 0; k < len; k++) data[k] = (uint8_t)rnd();
    uint32_t windows = 0;
    const uint32_t got = crc_by_windows(data.data(), base + off, base + off + len, &windows), want = crc_bits(data.data(), len);
    CHECK(got == want, "range at %llu of %llu bytes: by windows %08x, bit by bit %08x", (ull)off, (ull)len, got, want);
    CHECK(windows <= crc_segs_for(len), "range at %llu of %llu bytes touches %u windows, crc_segs_for gives %zu", (ull)off, (ull)len, windows, crc_segs_for(len));
  }
}

int main() {
  check_chunk_rule();
  check_run_fill();
  check_share_layout();
  check_crc_tables();
  check_crc_windows();
  if (g_fail) { printf("rle1_rules_check: %d checks failed\n", g_fail); return 1; }
  printf("rle1_rules_check ok\n");
  return 0;
}
