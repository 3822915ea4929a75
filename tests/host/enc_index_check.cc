// enc_index_check.cc — the host arithmetic of csrc/enc_index_plan.h (the compressor's block rows set at their bit offsets as index
// entries and line counts) checked by property on random row lists against a bit-by-bit walk, not by restating its formulas.
// Stand-alone: built with the host compiler under the address / undefined-behaviour sanitizers and run by
// tests/test_enc_index_host.py.  Exit 0 = all checks passed; a failing check prints itself and the program exits 1.
#include "enc_index_plan.h"
#include <stdio.h>
#include <string.h>
#include <vector>

using namespace cjs;

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_fail < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } g_fail++; } } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }
typedef unsigned long long ull;

// 0 .. max_rows rows: a block takes at least its 80 bits of magic and CRC and some more; `wide`: bit lengths near 2^32
static std::vector<EncRow> random_rows(size_t max_rows, bool wide) {
  std::vector<EncRow> r(rnd() % (max_rows + 1));
  for (EncRow& x : r) {
    x.bits = wide ? 0xFFFFFFFFu - (uint32_t)(rnd() % 1000) : 81u + (uint32_t)(rnd() % 8000000);
    x.crc = (uint32_t)rnd();
    x.size = 1u + (uint32_t)(rnd() % 46000000);
    x.newlines = (uint32_t)(rnd() % (x.size + 1ull));
  }
  return r;
}

static bool same_entry(const cjs_bz_index_entry& a, const cjs_bz_index_entry& b) {
  return a.bitpos == b.bitpos && a.end_bit == b.end_bit && a.size == b.size && a.crc == b.crc && a.level == b.level && a.reserved == b.reserved;
}

// The model: a stream laid out bit by bit.  Block k stands where block k - 1 ends, the first behind the 32 header bits; behind
// the last stand 48 bits of end-of-stream magic and 32 of stream CRC, and the stream is whole bytes.
struct Model { std::vector<uint64_t> start, end; uint64_t bytes; };
static Model lay_out(const std::vector<EncRow>& rows) {
  Model m;
  uint64_t bit = 0;
  bit += 8 * 4;                                           // 'B' 'Z' 'h' level
  for (const EncRow& r : rows) { m.start.push_back(bit); bit += r.bits; m.end.push_back(bit); }
  bit += 48; bit += 32;
  m.bytes = bit / 8 + (bit % 8 ? 1 : 0);
  return m;
}

static void one_case(size_t max_rows, bool wide) {
  const std::vector<EncRow> rows = random_rows(max_rows, wide);
  const int level = 1 + (int)(rnd() % 9);
  const Model m = lay_out(rows);
  // one piece
  std::vector<cjs_bz_index_entry> e1; std::vector<uint32_t> n1;
  const uint64_t end1 = enc_rows_append(e1, n1, rows.data(), rows.size(), ENC_FIRST_BIT, level);
  CHECK(e1.size() == rows.size() && n1.size() == rows.size(), "one entry and one count per row: %zu, %zu of %zu", e1.size(), n1.size(), rows.size());
  if (e1.size() != rows.size() || n1.size() != rows.size()) return;
  if (!rows.empty()) CHECK(e1[0].bitpos == 32, "the first block starts at bit %llu", (ull)e1[0].bitpos);
  for (size_t k = 0; k < rows.size(); k++) {
    CHECK(e1[k].bitpos == m.start[k] && e1[k].end_bit == m.end[k], "block %zu at [%llu, %llu), laid out at [%llu, %llu)", k, (ull)e1[k].bitpos, (ull)e1[k].end_bit,
          (ull)m.start[k], (ull)m.end[k]);
    if (k) CHECK(e1[k].bitpos == e1[k - 1].end_bit, "block %zu does not start where block %zu ends", k, k - 1);
    CHECK(e1[k].size == rows[k].size && e1[k].crc == rows[k].crc && e1[k].level == (uint32_t)level && e1[k].reserved == 0, "block %zu: size, crc, level, reserved", k);
    CHECK(n1[k] == rows[k].newlines, "block %zu: the count is row %zu's", k, k);
  }
  CHECK(end1 == (rows.empty() ? 32 : m.end.back()), "the bit behind the last row: %llu", (ull)end1);
  CHECK(enc_stream_bytes(end1) == m.bytes, "stream of %llu bytes, laid out in %llu", (ull)enc_stream_bytes(end1), (ull)m.bytes);
  if (rows.empty()) CHECK(enc_stream_bytes(end1) == 14, "the stream of no block is 14 bytes");
  // cut at random into pieces (the shards of a call, the steps of an encoder; empty pieces among them), each appended at the bit
  // the piece in front of it reached: the same tables
  std::vector<cjs_bz_index_entry> e2; std::vector<uint32_t> n2;
  std::vector<uint64_t> piece_start;
  uint64_t bit = ENC_FIRST_BIT;
  for (size_t at = 0;;) {
    const size_t take = rnd() % 3 == 0 ? 0 : (size_t)(rnd() % (rows.size() - at + 1));
    piece_start.push_back(bit);
    const size_t before = e2.size();
    bit = enc_rows_append(e2, n2, rows.data() + at, take, bit, level);
    CHECK(e2.size() == before + take && n2.size() == e2.size(), "a piece of %zu rows appends %zu entries, %zu counts in all", take, e2.size() - before, n2.size());
    if (!take) CHECK(bit == piece_start.back(), "an empty piece moves the bit");
    at += take;
    if (at == rows.size() && rnd() % 2) break;
  }
  CHECK(bit == end1, "pieces end at bit %llu, one piece at %llu", (ull)bit, (ull)end1);
  CHECK(e2.size() == e1.size() && n2 == n1, "pieces give %zu entries, one piece %zu", e2.size(), e1.size());
  for (size_t k = 0; k < e1.size() && k < e2.size(); k++) CHECK(same_entry(e1[k], e2[k]), "entry %zu differs between pieces and one piece", k);
  if (wide) CHECK(e1.size() < 2 || e1[1].end_bit > 0xFFFFFFFFull, "two blocks of ~2^32 bits end behind bit 2^32: %llu", (ull)e1[1].end_bit);
}

int main() {
  for (int it = 0; it < 3000; it++) one_case(40, false);
  for (int it = 0; it < 500; it++) one_case(3, false);       // (many with no row at all)
  for (int it = 0; it < 1500; it++) one_case(12, true);      // bit counts beyond 2^32
  {                                                          // a start bit beyond 2^32 is kept whole
    const EncRow r{100, 7, 5, 1};
    std::vector<cjs_bz_index_entry> e; std::vector<uint32_t> n;
    const uint64_t start = (1ull << 40) + 3;
    const uint64_t end = enc_rows_append(e, n, &r, 1, start, 9);
    CHECK(e.size() == 1 && e[0].bitpos == start && e[0].end_bit == start + 100 && end == start + 100, "a row at bit 2^40 + 3");
    CHECK(enc_stream_bytes(32) == 14 && enc_stream_bytes(33) == 15 && enc_stream_bytes(40) == 15 && enc_stream_bytes(41) == 16, "the last byte is padded");
  }
  if (g_fail) { printf("enc_index_check: %d checks failed\n", g_fail); return 1; }
  printf("enc_index_check ok\n");
  return 0;
}
