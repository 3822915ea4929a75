// enc_pieces_check -- the rule of the compress pipeline's pieces (csrc/enc_pieces.h) on the host, without HIP: when a call goes
// in one piece, the default threshold by its constant, the tiling of [0, cnt) for cnt 1..64, the piece sizes of the small counts
// by name, and no overflow at the largest count.  A stand-alone program; the test builds it under the address and
// undefined-behaviour sanitizers.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "enc_pieces.h"

using namespace cjs;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

// the sizes of the runs the pipeline's loop makes of cnt blocks
static std::vector<uint32_t> sizes(uint32_t cnt, uint32_t cap, uint64_t min_bytes, bool stage_times = false, bool has_tail = true) {
  const TablePieces p = table_pieces(cnt, cap, min_bytes, stage_times, has_tail);
  std::vector<uint32_t> out;
  uint64_t at = 0;
  for (uint32_t i = 0; i < table_piece_count(cnt, p); i++) {
    uint32_t k0, kc;
    table_piece(cnt, p, i, k0, kc);
    CHECK(k0 == at);                   // in order, nothing left out, nothing twice
    out.push_back(kc);
    at += kc;
  }
  CHECK(at == cnt);
  return out;
}

static void check_one_piece() {
  const uint32_t cap9 = 899981, cap1 = 99981;
  for (uint32_t cnt : {1u, 2u, 5u, 444u, 445u, 1194u, 100000u}) {
    for (uint32_t cap : {cap1, cap9}) {
      for (uint64_t min_bytes : {(uint64_t)1, (uint64_t)ENC_PIECE_BYTES, ~(uint64_t)0}) {
        const bool below = (uint64_t)cnt * cap < min_bytes;
        for (int st = 0; st < 2; st++)
          for (int tail = 0; tail < 2; tail++) {
            const TablePieces p = table_pieces(cnt, cap, min_bytes, st != 0, tail != 0);
            const bool one = st || !tail || below;
            CHECK(p.pieces == (one ? 1u : 4u));
            CHECK(p.per == (cnt + p.pieces - 1) / p.pieces);
            if (one) { CHECK(p.per == cnt && table_piece_count(cnt, p) == 1); }
          }
      }
    }
  }
  // no block: no run, whatever the rest says
  for (uint64_t min_bytes : {(uint64_t)0, (uint64_t)1, (uint64_t)ENC_PIECE_BYTES}) {
    const TablePieces p = table_pieces(0, cap9, min_bytes, false, true);
    CHECK(p.per == 0 && table_piece_count(0, p) == 0);
  }
  // cnt * cap == min_bytes is not below it
  CHECK(table_pieces(10, 100, 1000, false, true).pieces == 4 && table_pieces(10, 100, 1001, false, true).pieces == 1);
}

static void check_default_threshold() {
  CHECK(ENC_PIECE_BYTES == 400000000ull && ENC_PIECES == 4);
  const uint32_t cap9 = 9 * 100000 - 19;
  CHECK(444ull * cap9 < ENC_PIECE_BYTES && 445ull * cap9 >= ENC_PIECE_BYTES);
  CHECK(table_pieces(444, cap9, ENC_PIECE_BYTES, false, true).pieces == 1);
  CHECK(table_pieces(445, cap9, ENC_PIECE_BYTES, false, true).pieces == 4);
  CHECK(sizes(444, cap9, ENC_PIECE_BYTES) == std::vector<uint32_t>({444}));
  CHECK(sizes(445, cap9, ENC_PIECE_BYTES) == std::vector<uint32_t>({112, 112, 112, 109}));
  CHECK(sizes(1194, cap9, ENC_PIECE_BYTES) == std::vector<uint32_t>({299, 299, 299, 297}));      // 2^30 bytes of text at level 9
}

static void check_tiling() {
  for (uint32_t cnt = 1; cnt <= 64; cnt++) {
    const TablePieces p = table_pieces(cnt, 99981, 1, false, true);
    CHECK(p.pieces == 4 && p.per == (cnt + 3) / 4);
    const std::vector<uint32_t> s = sizes(cnt, 99981, 1);          // (tiles [0, cnt) in order: checked in there)
    CHECK(!s.empty() && s.size() <= 4);
    CHECK(s.size() == (cnt + p.per - 1) / p.per);
    for (size_t i = 0; i < s.size(); i++) {
      CHECK(s[i] >= 1);
      if (i + 1 < s.size()) CHECK(s[i] == p.per); else CHECK(s[i] <= p.per);
    }
  }
}

static void check_named_counts() {
  struct { uint32_t cnt; std::vector<uint32_t> want; } cases[] = {
    {1, {1}}, {2, {1, 1}}, {3, {1, 1, 1}}, {4, {1, 1, 1, 1}}, {5, {2, 2, 1}}, {6, {2, 2, 2}}, {7, {2, 2, 2, 1}}, {8, {2, 2, 2, 2}},
    {9, {3, 3, 3}}, {10, {3, 3, 3, 1}}, {13, {4, 4, 4, 1}}};
  for (const auto& c : cases) CHECK(sizes(c.cnt, 99981, 1) == c.want);
}

static void check_no_overflow() {
  const uint32_t cnt = 0xFFFFFFFFu, cap9 = 899981;
  // 2^32 - 1 blocks of level 9 are 3.8e15 bytes: above the default threshold, below one of 2^52
  CHECK(table_pieces(cnt, cap9, ENC_PIECE_BYTES, false, true).pieces == 4);
  CHECK(table_pieces(cnt, cap9, 1ull << 52, false, true).pieces == 1);
  CHECK(table_pieces(cnt, 0xFFFFFFFFu, 0xFFFFFFFE00000001ull, false, true).pieces == 4);          // cnt * cap exactly
  CHECK(table_pieces(cnt, 0xFFFFFFFFu, 0xFFFFFFFE00000002ull, false, true).pieces == 1);
  const TablePieces p = table_pieces(cnt, cap9, 1, false, true);
  CHECK(p.per == 0x40000000u && table_piece_count(cnt, p) == 4);
  CHECK(sizes(cnt, cap9, 1) == std::vector<uint32_t>({0x40000000u, 0x40000000u, 0x40000000u, 0x3FFFFFFFu}));
  const TablePieces one = table_pieces(cnt, cap9, 1, true, true);
  CHECK(one.per == cnt && table_piece_count(cnt, one) == 1);
  CHECK(sizes(cnt, cap9, 1, true) == std::vector<uint32_t>({cnt}));
}

int main() {
  check_one_piece();
  check_default_threshold();
  check_tiling();
  check_named_counts();
  check_no_overflow();
  printf("enc_pieces_check ok\n");
  return 0;
}
