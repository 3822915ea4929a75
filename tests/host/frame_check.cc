// frame_check.cc — the host arithmetic of csrc/bz_frame.h against bit-by-bit models.  Stand-alone: built with the host compiler
// (and the address / undefined-behaviour sanitizers where they link) and run by tests/test_frame_host.py.  Exit 0 = all checks
// passed; a failing check prints itself and the program exits 1.
#include "bz_frame.h"
#include <stdio.h>
#include <stdlib.h>
#include <vector>

using namespace cjs;

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_fail < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } g_fail++; } } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }

static int get_bit(const uint8_t* p, uint64_t b) { return (p[b >> 3] >> (7 - (b & 7))) & 1; }
static void or_bit(uint8_t* p, uint64_t b, int v) { if (v) p[b >> 3] |= (uint8_t)(0x80 >> (b & 7)); }

struct Meta { uint64_t bits; uint32_t blocks, crc_fold; };      // the fields of cjs_shard_meta that shard_layout reads

// One (pos, nbits): the source holds exactly the bytes of its bits plus the 9 readable bytes of slack the contract states (heap
// memory of exactly that size: the sanitizer sees a read past it).  dst: zero inside the range (the stitch's buffer comes from
// calloc, the interior is stored, the ends are OR-ed), random bits on both sides of it, which must survive.
static void merge_case(uint64_t pos, uint64_t nbits) {
  const size_t src_bytes = (size_t)((nbits + 7) / 8) + 9;
  uint8_t* src = (uint8_t*)malloc(src_bytes);
  for (size_t i = 0; i < src_bytes; i++) src[i] = (uint8_t)rnd();
  const size_t dst_bytes = (size_t)((pos + nbits + 7) / 8) + 2;
  std::vector<uint8_t> base(dst_bytes);
  for (auto& x : base) x = (uint8_t)rnd();
  for (uint64_t b = pos; b < pos + nbits; b++) base[b >> 3] &= (uint8_t)~(0x80 >> (b & 7));
  std::vector<uint8_t> want = base;
  for (uint64_t b = 0; b < nbits; b++) or_bit(want.data(), pos + b, get_bit(src, b));
  // edges = 0 alone: only whole bytes inside the range, and exactly the model's bytes there
  std::vector<uint8_t> inner = base;
  funnel_merge(inner.data(), pos, src, nbits, 0);
  const uint64_t j0 = (pos + 7) >> 3, j1 = (pos + nbits) >> 3;
  for (size_t j = 0; j < dst_bytes; j++) {
    const bool in = j >= j0 && j < j1;
    CHECK(inner[j] == (in ? want[j] : base[j]), "interior: pos %llu nbits %llu byte %zu: %02x", (unsigned long long)pos, (unsigned long long)nbits, j, inner[j]);
  }
  // edges = 1 alone: only the partial bytes at the two ends
  std::vector<uint8_t> ends = base;
  funnel_merge(ends.data(), pos, src, nbits, 1);
  for (size_t j = 0; j < dst_bytes; j++) {
    const bool in = j >= j0 && j < j1;
    CHECK(ends[j] == (in ? base[j] : want[j]), "edges: pos %llu nbits %llu byte %zu: %02x want %02x", (unsigned long long)pos, (unsigned long long)nbits, j, ends[j], want[j]);
  }
  // both, in the order the stitch runs them
  funnel_merge(inner.data(), pos, src, nbits, 1);
  CHECK(inner == want, "combined: pos %llu nbits %llu", (unsigned long long)pos, (unsigned long long)nbits);
  free(src);
}

static void check_funnel_merge() {
  for (uint64_t ph = 0; ph < 8; ph++)
    for (uint64_t nbits = 1; nbits <= 80; nbits++) { merge_case(ph, nbits); merge_case(64 + ph, nbits); }
  for (int i = 0; i < 4000; i++) merge_case(rnd() % 4096, 1 + rnd() % 4096);
}

static void check_crc_fold() {
  CHECK(crc_fold(0x80000001u, 0) == 0x00000003u, "crc_fold rotates left by one");
  CHECK(crc_fold(0, 0xDEADBEEFu) == 0xDEADBEEFu, "crc_fold from 0");
  const uint32_t counts[] = {0, 1, 2, 31, 32, 33, 63, 64, 65, 100};
  for (uint32_t na : counts)
    for (uint32_t nb : counts) {
      std::vector<uint32_t> crcs(na + nb);
      for (auto& x : crcs) x = (uint32_t)rnd();
      uint32_t whole = 0, a = 0, b = 0;
      for (uint32_t x : crcs) whole = crc_fold(whole, x);
      for (uint32_t k = 0; k < na; k++) a = crc_fold(a, crcs[k]);
      for (uint32_t k = 0; k < nb; k++) b = crc_fold(b, crcs[na + k]);
      CHECK(crc_fold_join(crc_fold_join(0, na, a), nb, b) == whole, "crc_fold_join over a split %u + %u", na, nb);
      CHECK(crc_fold_join(a, 0, 0) == a, "a part without blocks leaves the CRC as it is");
    }
}

static void check_shard_layout() {
  // ranks without blocks at the front, in the middle and at the end; a model that walks the blocks one by one
  const uint32_t shapes[][6] = {{0, 3, 0, 2, 0, 0}, {0, 0, 33, 0, 32, 0}, {5, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 7}, {0, 0, 0, 0, 0, 0}, {1, 1, 1, 1, 1, 1}};
  for (const auto& shape : shapes) {
    Meta m[6];
    uint32_t whole = 0; uint64_t bit = 32, want_start[6]; int want_writer = 0;
    for (int r = 0; r < 6; r++) {
      m[r] = Meta{0, shape[r], 0};
      want_start[r] = bit;
      for (uint32_t k = 0; k < shape[r]; k++) {
        const uint32_t crc = (uint32_t)rnd(), len = 100 + (uint32_t)(rnd() % 5000);
        m[r].bits += len; bit += len;
        m[r].crc_fold = crc_fold(m[r].crc_fold, crc); whole = crc_fold(whole, crc);
      }
      if (shape[r]) want_writer = r;
    }
    for (int rank = 0; rank < 6; rank++) {
      uint64_t start = 0, total = 0, starts[6]; uint32_t scrc = 1; int writer = -1;
      shard_layout(m, 6, rank, start, total, scrc, writer, starts);
      CHECK(start == want_start[rank] && total == bit && scrc == whole && writer == want_writer, "shard_layout rank %d: start %llu total %llu crc %08x writer %d",
            rank, (unsigned long long)start, (unsigned long long)total, scrc, writer);
      for (int r = 0; r < 6; r++) CHECK(starts[r] == want_start[r], "shard_layout starts[%d]", r);
      uint64_t s2 = 0, t2 = 0; uint32_t c2 = 0; int w2 = 0;
      shard_layout(m, 6, rank, s2, t2, c2, w2);               // without the optional array
      CHECK(s2 == start && t2 == total && c2 == scrc && w2 == writer, "shard_layout without starts[]");
    }
  }
}

static void check_put_trailer() {
  for (uint64_t bit = 0; bit < 40; bit++) {
    const uint32_t crc = (uint32_t)rnd();
    const size_t nbytes = (size_t)((bit + 80 + 7) / 8);
    uint8_t* got = (uint8_t*)calloc(nbytes, 1);             // exactly the bytes the trailer reaches
    std::vector<uint8_t> want(nbytes, 0);
    for (uint64_t b = 0; b < bit; b++) { const int v = (int)(rnd() & 1); or_bit(got, b, v); or_bit(want.data(), b, v); }
    const uint64_t magic = 0x177245385090ull;
    for (int i = 0; i < 48; i++) or_bit(want.data(), bit + i, (int)((magic >> (47 - i)) & 1));
    for (int i = 0; i < 32; i++) or_bit(want.data(), bit + 48 + i, (int)((crc >> (31 - i)) & 1));
    put_trailer(got, bit, crc);
    for (size_t j = 0; j < nbytes; j++) CHECK(got[j] == want[j], "put_trailer at bit %llu byte %zu", (unsigned long long)bit, j);
    free(got);
  }
}

int main() {
  check_funnel_merge();
  check_crc_fold();
  check_shard_layout();
  check_put_trailer();
  if (g_fail) { printf("frame_check: %d checks failed\n", g_fail); return 1; }
  printf("frame_check ok\n");
  return 0;
}
