// huff_rules_check.cc — the host-visible rules of the entropy stage, csrc/huff_rules.h, checked against the oracle: the code-length
// allocator (pass 1 and the control flow of passes 2 and 3 with serial callables) against cjs_oracle_huff_alloc, the rank-sort key
// against cjs_oracle_huff_lengths, a block written item by item (header, selectors, tables, canonical codes) against
// cjs_oracle_bzip2_block_bits bit for bit, the geometry and the workspace layout against the literal formulas they replaced, and
// the bit splitter against a bit-by-bit writer.
// Stand-alone: built with the host compiler under the address / undefined-behaviour sanitizers, linked with oracle/cjs_oracle.c, and
// run by tests/test_huff_rules_host.py.  Exit 0 = all checks passed; a failing check prints itself and the program exits 1.
#include "huff_rules.h"
#include "cjs_oracle.h"
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <vector>

using namespace cjs;

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_fail < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } g_fail++; } } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }
static uint32_t below(uint32_t n) { return (uint32_t)(rnd() % n); }
typedef unsigned long long ull;

// ---- the allocator with serial callables: what ha_passes23_wave does with ballots and masked stores
static void alloc_serial(int* a, int len, int maxlen) {
  if (!ha_pass1(a, len)) return;
  ha_passes23(len, maxlen, ha_mod(a[0], len),
              [&](int limit, int lo) { return ha_first(a, len, limit, lo); },
              [&](int lo, int hi, int x) { for (int i = lo; i <= hi; i++) a[i] = x; },
              [&](int i) { return a[i]; });
}
// which branch of pass 3 a vector takes (for the coverage counts only): pass 2 as the header's comment states it
static bool takes_relocation(const int* sorted, int len, int maxlen) {
  std::vector<int> a(sorted, sorted + len);
  if (!ha_pass1(a.data(), len)) return false;
  int reloc = len - 2;
  for (int depth = 1; depth < maxlen - 1 && reloc > 1; depth++) reloc = ha_first(a.data(), len, reloc - 1, 0);
  return ha_mod(a[0], len) < reloc;
}

static void gen_freq(int family, int n, std::vector<uint32_t>& f) {
  f.assign(n, 0);
  switch (family) {
    case 0: { const uint32_t v = 1 + below(1000); for (auto& x : f) x = v; break; }                              // uniform
    case 1: for (auto& x : f) x = 1; break;                                                                     // all ones
    case 2: for (auto& x : f) x = below(4) ? 0 : 1 + below(5000); break;                                        // many zeros
    case 3: {                                                                                                   // geometric, capped
      const double ratio = 1.3 + 0.67 * (double)below(1001) / 1000.0;
      double v = 1.0 + below(3);
      for (auto& x : f) { x = (uint32_t)(v < 900000.0 ? v : 900000.0); v *= ratio; if (v > 4e6) v = 4e6; }
      for (int i = n - 1; i > 0; i--) std::swap(f[i], f[below((uint32_t)i + 1)]);
      break;
    }
    default: for (auto& x : f) x = below(1u << (1 + below(20))); break;                                         // wide random
  }
}

static void check_allocator() {
  const int CASES = 63000;
  int at_limit = 0, relocated = 0;
  std::vector<uint32_t> f;
  for (int c = 0; c < CASES; c++) {
    const int n = c < 258 * 5 ? 1 + c / 5 : 1 + (int)below(258);          // every n in every family, then random n
    const int family = c % 5, maxlen = c % 7 == 3 ? 32 : MAX_BITS;
    gen_freq(family, n, f);
    std::vector<uint32_t> sorted(f);
    std::sort(sorted.begin(), sorted.end());
    std::vector<int32_t> want(sorted.begin(), sorted.end());
    std::vector<int> got(sorted.begin(), sorted.end());
    if (takes_relocation(got.data(), n, maxlen)) relocated++;
    cjs_oracle_huff_alloc(want.data(), n, maxlen);
    alloc_serial(got.data(), n, maxlen);
    bool same = true;
    for (int i = 0; i < n; i++) same = same && want[i] == got[i];
    CHECK(same, "allocator: case %d (family %d, n %d, limit %d) differs from the oracle", c, family, n, maxlen);
    if (got[0] == maxlen) at_limit++;
    if (maxlen != MAX_BITS) continue;
    // the rank-sort key: symbols by (frequency, index), lengths back by the key's index
    uint8_t want_len[MAXSYM], got_len[MAXSYM];
    cjs_oracle_huff_lengths(f.data(), n, want_len);
    std::vector<uint32_t> key(n);
    for (int i = 0; i < n; i++) key[i] = rank_key(f[i], (uint32_t)i);
    std::sort(key.begin(), key.end());
    std::vector<int> a(n);
    for (int i = 0; i < n; i++) a[i] = (int)(key[i] >> 9);
    alloc_serial(a.data(), n, MAX_BITS);
    for (int i = 0; i < n; i++) got_len[key[i] & 0x1ff] = (uint8_t)a[i];
    CHECK(memcmp(want_len, got_len, n) == 0, "lengths by rank key: case %d (family %d, n %d) differs from the oracle", c, family, n);
  }
  CHECK(at_limit * 10 >= CASES, "allocator: only %d of %d cases reach the limit", at_limit, CASES);
  CHECK(relocated >= 1000, "allocator: only %d cases take the relocation branch", relocated);
  printf("allocator: %d cases, %d with the longest code at the limit, %d through the relocation branch\n", CASES, at_limit, relocated);
}

// ---- a block, item by item, through a serial bit writer
struct Bits {
  std::vector<uint8_t> bytes; uint64_t n = 0;
  void put(BitItem it) {
    for (int i = (int)it.nbits - 1; i >= 0; i--, n++) {
      if ((n & 7) == 0) bytes.push_back(0);
      if ((it.val >> i) & 1) bytes[n >> 3] |= (uint8_t)(0x80 >> (n & 7));
    }
  }
};

static void check_block(uint32_t npos, uint32_t asz, bool scattered) {
  const uint32_t n = asz + 2;
  // symbols whose statistics drift along the block, so that the tables differ; EOB last
  std::vector<uint16_t> A(npos);
  for (uint32_t i = 0; i + 1 < npos; i++) {
    const uint32_t phase = (i * 4 / npos) & 3, r = below(100);
    uint32_t s = r < 40 ? below(2) : r < 85 ? (phase * 7 + below(9)) % (asz + 1) : below(asz + 1);
    A[i] = (uint16_t)s;
  }
  A[npos - 1] = (uint16_t)(asz + 1);
  uint8_t used[256] = {0};
  if (!scattered) for (uint32_t i = 0; i < asz; i++) used[i] = 1;
  else {                                                                // asz bytes of a shuffled 0..255
    uint8_t perm[256];
    for (int i = 0; i < 256; i++) perm[i] = (uint8_t)i;
    for (int i = 255; i > 0; i--) std::swap(perm[i], perm[below((uint32_t)i + 1)]);
    for (uint32_t k = 0; k < asz; k++) used[perm[k]] = 1;
  }
  const uint32_t crc = (uint32_t)rnd(), pidx = below(1u << 24);
  uint8_t* want = nullptr; uint64_t want_bits = 0;
  const int rc = cjs_oracle_bzip2_block_bits(A.data(), (int)npos, (int)asz, used, crc, pidx, &want, &want_bits);
  CHECK(rc == 0, "oracle block bits: rc %d", rc);
  if (rc) return;
  std::vector<uint8_t> sel(groups_for(npos) + 2), lens(lens_row_bytes());
  const uint32_t ng = (uint32_t)cjs_oracle_huff_groups(A.data(), (int)npos, (int)asz, sel.data(), lens.data());
  const uint32_t nsel = groups_for(npos);
  CHECK((int)ng == huff_target(npos), "npos %u: the oracle uses %u tables, huff_target says %d", npos, ng, huff_target(npos));
  // used map as pack_block holds it: [0] = ranges in use, [1 + r] = bytes of range r
  uint32_t used16[17] = {0};
  for (uint32_t v = 0; v < 256; v++) if (used[v]) { used16[1 + (v >> 4)] |= 0x8000u >> (v & 15); used16[0] |= 0x8000u >> (v >> 4); }
  const uint32_t nranges = (uint32_t)__builtin_popcount(used16[0]);
  Bits w;
  for (uint32_t i = 0; i < HEADER_ITEMS; i++) w.put(header_item(i, crc, pidx, used16[0], used16 + 1, ng, nsel));
  uint32_t sel_bits = 0, tab_bits = 0, data_bits = 0;
  uint8_t M[MAXTAB];
  for (uint32_t i = 0; i < ng; i++) M[i] = (uint8_t)i;
  for (uint32_t g = 0; g < nsel; g++) {                                 // the selector's MTF position, serially
    uint32_t j = 0;
    while (M[j] != sel[g]) j++;
    for (uint32_t k = j; k > 0; k--) M[k] = M[k - 1];
    M[0] = sel[g];
    w.put(selector_item(j)); sel_bits += selector_item(j).nbits;
  }
  std::vector<uint32_t> codes(codes_row_elems());
  for (uint32_t t = 0; t < ng; t++) {
    const uint8_t* L = lens.data() + t * MAXSYM;
    for (uint32_t s = 0; s < n; s++) { const BitItem it = table_item(L[s], s ? L[s - 1] : L[s], s == 0); w.put(it); tab_bits += it.nbits; }
    canonical_codes(L, (int)n, codes.data() + t * MAXSYM);
  }
  for (uint32_t i = 0; i < npos; i++) {
    const uint32_t t = sel[i / GSZ], s = A[i];
    w.put(BitItem{codes[t * MAXSYM + s], lens[t * MAXSYM + s]}); data_bits += lens[t * MAXSYM + s];
  }
  CHECK(w.n == want_bits, "block npos %u asz %u: %llu bits, the oracle has %llu", npos, asz, (ull)w.n, (ull)want_bits);
  CHECK(w.n == block_bits(nranges, sel_bits, tab_bits, data_bits), "block npos %u asz %u: %llu bits written, block_bits says %u", npos, asz, (ull)w.n,
        block_bits(nranges, sel_bits, tab_bits, data_bits));
  CHECK(w.n == want_bits && memcmp(w.bytes.data(), want, (size_t)((want_bits + 7) / 8)) == 0, "block npos %u asz %u scattered %d: bits differ from the oracle's", npos, asz, (int)scattered);
  cjs_oracle_free(want);
}
static void check_blocks() {
  static const uint32_t NPOS[] = {2, 49, 50, 51, 199, 200, 201, 599, 600, 1199, 1200, 2399, 2400, 2401, 3999, 4000, 4001};
  static const uint32_t ASZ[] = {1, 2, 17, 255, 256};
  int blocks = 0;
  for (int rep = 0; rep < 2; rep++)
    for (uint32_t npos : NPOS) for (uint32_t asz : ASZ) for (int sc = 0; sc < 2; sc++) { check_block(npos, asz, sc != 0); blocks++; }
  printf("blocks: %d written item by item\n", blocks);
}

// ---- geometry and workspace against the literal formulas that stood in huff.hip, huff.h and stages.hip
static size_t parent_bytes_needed(size_t max_blocks, uint32_t stride) {
  size_t b = 0;
  auto add = [&](size_t n) { b += (n + 255) & ~(size_t)255; };
  const size_t ss = (((size_t)stride + 1 + 49) / 50 + 63) & ~(size_t)63;
  add(max_blocks * ss); add(max_blocks * ss); add(max_blocks * ss * 2);
  add(max_blocks * 6 * 258); add(max_blocks * 6 * 258 * 4);
  add(max_blocks * 4); add(max_blocks * 4); add((max_blocks + 1) * 8); add(64);
  add(max_blocks * 4); add(max_blocks * (ss / 80 + 2) * 4);
  add(max_blocks * 6 * 264); add(max_blocks * 6 * 260 * 4);
  return b + 4096;
}
static void check_geometry_one(uint32_t stride) {
  const uint32_t maxpos = stride + 1;                                    // a block of `stride` bytes yields up to stride + 1 symbols
  const size_t ss = sel_stride_for(stride), ts = tile_stride_for(ss);
  const uint32_t nsel = groups_for(maxpos);
  CHECK((uint64_t)nsel * GSZ >= maxpos && (uint64_t)(nsel - 1) * GSZ < maxpos, "groups_for(%u) = %u", maxpos, nsel);
  CHECK(ss >= nsel && ss % 64 == 0, "sel_stride_for(%u) = %llu for %u groups", stride, (ull)ss, nsel);
  CHECK(ss <= (((size_t)stride + 1 + 49) / 50 + 63) / 64 * 64, "sel_stride_for(%u) = %llu exceeds the literal formula", stride, (ull)ss);
  const uint32_t ntile = tiles_for_groups(nsel);
  CHECK((uint64_t)ntile * PD_GROUPS >= nsel && (uint64_t)(ntile - 1) * PD_GROUPS < nsel, "tiles_for_groups(%u) = %u", nsel, ntile);
  CHECK(ts - 1 >= ntile, "tile_stride_for(%llu) = %llu: the grid of pack_data (one less) misses one of %u tiles", (ull)ss, (ull)ts, ntile);
  CHECK(ts <= ss / 80 + 2, "tile_stride_for(%llu) = %llu exceeds the literal formula", (ull)ss, (ull)ts);
  const uint32_t ga = hs_assign_grid(stride), gc = hs_count_grid(stride);
  CHECK((uint64_t)ga * HS_STEPS * AS_GROUPS >= nsel && ga <= (nsel + 2047) / 2048, "hs_assign_grid(%u) = %u for %u groups", stride, ga, nsel);
  CHECK((uint64_t)gc * HS_CNT >= maxpos && gc <= (maxpos + 131071) / 131072, "hs_count_grid(%u) = %u for %u symbols", stride, gc, maxpos);
  static const size_t BLOCKS[] = {0, 1, 2, 7, 112, 513, 4096, 20000};
  // rows per block as HuffWork::view steps them (0: not stepped per block)
  const size_t row[HB_COUNT] = {ss, ss, ss, lens_row_bytes(), codes_row_elems(), 1, 1, 0, 0, 1, ts, wl_row_bytes(), wfreq_row_elems()};
  for (size_t mb : BLOCKS) {
    const HuffLayout L = huff_layout(mb, stride);
    CHECK(huff_layout_bytes(L) == parent_bytes_needed(mb, stride), "bytes_needed(%llu, %u) = %llu, was %llu", (ull)mb, stride, (ull)huff_layout_bytes(L), (ull)parent_bytes_needed(mb, stride));
    size_t used = 0;                                                     // a sequential carve, each buffer at a 256-byte boundary
    for (int i = 0; i < HB_COUNT; i++) {
      used += (L.n[i] * HUFF_ELEM_BYTES[i] + 255) & ~(size_t)255;
      if (row[i]) CHECK(L.n[i] == mb * row[i], "buffer %d of (%llu, %u): %llu elements, view steps %llu per block", i, (ull)mb, stride, (ull)L.n[i], (ull)row[i]);
    }
    CHECK(used <= huff_layout_bytes(L), "carve of (%llu, %u) takes %llu of %llu bytes", (ull)mb, stride, (ull)used, (ull)huff_layout_bytes(L));
    CHECK(L.n[HB_BITOFF] == mb + 1 && L.n[HB_SCALARS] >= 5, "bitoff / scalars of (%llu, %u)", (ull)mb, stride);
    CHECK(L.sel_stride == ss && L.tile_stride == ts, "strides of (%llu, %u)", (ull)mb, stride);
  }
}
static void check_geometry() {
  for (uint32_t stride = 1; stride <= 2000; stride++) check_geometry_one(stride);
  for (uint32_t level = 1; level <= 9; level++) check_geometry_one(level * 100000 - 19);
  check_geometry_one(1048574);
  // the frame and the capacity rule against the numbers that stood in the kernels
  for (int i = 0; i < 20000; i++) {
    const uint64_t end = rnd() % (1ull << (1 + below(40))), cap = rnd() % (1ull << (1 + below(38))), tb = below(2) ? STREAM_TRAILER_BITS : 0;
    CHECK(stream_too_small(end, tb, cap) == ((end + tb + 7) / 8 + 8 > cap), "stream_too_small(%llu, %llu, %llu)", (ull)end, (ull)tb, (ull)cap);
    uint64_t bytes = (end + tb + 7) / 8 + 16; if (bytes > cap) bytes = cap;
    CHECK(stream_zeroed_bytes(end, tb, cap) == bytes, "stream_zeroed_bytes(%llu, %llu, %llu)", (ull)end, (ull)tb, (ull)cap);
    CHECK(framed_bits(end) == 112 + end && STREAM_HEADER_BITS == 32 && STREAM_TRAILER_BITS == 80, "framed_bits(%llu)", (ull)end);
  }
}

// ---- the bit splitter against a bit-by-bit writer
static void check_splitter() {
  for (uint32_t off = 0; off < 64; off++) for (uint32_t len = 1; len <= 64; len++) {
    const uint64_t val = rnd(), bit = 64 * (uint64_t)below(3) + off;
    uint8_t want[40] = {0}; uint32_t words[10] = {0};
    for (uint32_t i = 0; i < len; i++) if ((val >> (len - 1 - i)) & 1) want[(bit + i) >> 3] |= (uint8_t)(0x80 >> ((bit + i) & 7));
    uint64_t prev_w = 0; int pieces = 0;
    split_bits(bit, val, len, [&](uint64_t w, uint32_t piece) {
      CHECK(w < 10 && (pieces == 0 || w == prev_w + 1), "split_bits(%llu, len %u): word %llu after %llu", (ull)bit, len, (ull)w, (ull)prev_w);
      if (w < 10) words[w] |= piece;
      prev_w = w; pieces++;
    });
    bool same = true;
    for (int i = 0; i < 40; i++) same = same && want[i] == (uint8_t)(words[i >> 2] >> (24 - 8 * (i & 3)));
    CHECK(same && pieces <= 3, "split_bits(%llu, len %u) differs from the bit-by-bit writer (%d pieces)", (ull)bit, len, pieces);
  }
  // the trailer as put_trailer_words splits it, against put_trailer of bz_frame.h
  for (uint64_t bit = 0; bit < 128; bit++) {
    const uint32_t crc = (uint32_t)rnd();
    uint8_t want[32] = {0}; uint32_t words[8] = {0};
    put_trailer(want, bit, crc);
    const auto put = [&](uint64_t w, uint32_t piece) { words[w] |= piece; };
    split_bits(bit, MAGIC_END, 48, put);
    split_bits(bit + 48, crc, 32, put);
    bool same = true;
    for (int i = 0; i < 32; i++) same = same && want[i] == (uint8_t)(words[i >> 2] >> (24 - 8 * (i & 3)));
    CHECK(same, "trailer at bit %llu differs from put_trailer", (ull)bit);
  }
}

int main() {
  check_allocator();
  check_blocks();
  check_geometry();
  check_splitter();
  if (g_fail) { printf("huff_rules_check: %d checks failed\n", g_fail); return 1; }
  printf("huff_rules_check ok\n");
  return 0;
}
