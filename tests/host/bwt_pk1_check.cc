// The narrow phase-1 record of the packed cyclic round 1 (csrc/bwt_rules.h: pk1_record, pk1_of, pk1_b2) and the fields that
// bwt_phase2_records takes back from the text (pk_key_of_text, pk_bytes01_of_text, pk_prev_of_text), on the host compiler:
//   * the 32-bit record round-trips every position up to 2^20 - 3 (the last position of the longest block) with every byte 2,
//     and no field reaches into the other;
//   * pk_pos reads the same position from the 8-byte record, from its narrowed form and from a record built narrow;
//   * narrowing a pk_record keeps byte 2 (its top byte) whatever the other four key bytes and the parity bit are;
//   * records order as (byte 2, position), which is what the last LSD pass relies on;
//   * the key formed from eight text bytes is the key that gen_key packs into the 8-byte record for the same suffix.
// Stand-alone program, no HIP.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "bwt_rules.h"

using namespace cjs;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { if (fails++ < 20) fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); } } while (0)

static uint64_t rnd_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rnd_state ^= rnd_state << 13; rnd_state ^= rnd_state >> 7; rnd_state ^= rnd_state << 17; return rnd_state; }

int main() {
  static_assert(PK1_B2_SHIFT == RANK_BITS && PK1_B2_SHIFT + 8 <= 32, "byte 2 sits on the position and fits the word");
  static_assert(pk1_record(0xFFu, 0u) == 0x0FF00000u && pk1_record(0u, PK_POS_MASK) == PK_POS_MASK, "fields do not overlap");
  const uint32_t max_pos = BWT_MAX_STRIDE - 1u;                  // 2^20 - 3
  CHECK(max_pos == (1u << 20) - 3u);
  // every position with every byte 2
  uint64_t acc = 0;
  for (uint32_t b2 = 0; b2 < 256u; b2++)
    for (uint32_t pos = 0; pos <= max_pos; pos++) {
      const uint32_t r = pk1_record(b2, pos);
      if (pk_pos(r) != pos || pk1_b2(r) != b2 || (r >> 28) != 0u) { CHECK(pk_pos(r) == pos); CHECK(pk1_b2(r) == b2); CHECK((r >> 28) == 0u); }
      acc += r;
    }
  CHECK(acc != 0);
  // order: (byte 2, position)
  for (int i = 0; i < 200000; i++) {
    const uint32_t b2a = (uint32_t)rnd() & 255u, b2b = (uint32_t)rnd() & 255u, pa = (uint32_t)(rnd() % (max_pos + 1u)), pb = (uint32_t)(rnd() % (max_pos + 1u));
    const bool lt = b2a < b2b || (b2a == b2b && pa < pb);
    CHECK((pk1_record(b2a, pa) < pk1_record(b2b, pb)) == lt);
  }
  // pk_pos on both layouts, narrowing keeps byte 2 and the position
  for (int i = 0; i < 2000000; i++) {
    const uint64_t key40 = rnd() & 0xFFFFFFFFFFull;
    const uint32_t parity = (uint32_t)rnd() & 1u, pos = i < 8 ? (i & 1 ? max_pos - (uint32_t)(i >> 1) : (uint32_t)(i >> 1)) : (uint32_t)(rnd() % (max_pos + 1u));
    const uint64_t wide = pk_record(key40, parity, pos);
    const uint32_t narrow = pk1_of(wide);
    CHECK(pk_pos(wide) == pos);
    CHECK(pk_pos(narrow) == pos);
    CHECK(pk_pos(wide) == pk_pos(narrow));
    CHECK(pk1_b2(narrow) == (uint32_t)(key40 >> 32));
    CHECK(narrow == pk1_record((uint32_t)(key40 >> 32), pos));
    CHECK(pk_pos(pk2_record((uint32_t)rnd(), (uint32_t)rnd() & RANK_MASK, (uint32_t)rnd() & 255u, pos)) == pos);      // and of the phase-2 record
  }
  // the fields out of the eight text bytes around a suffix: t = text[p - 1 .. p + 6], first byte lowest
  for (int i = 0; i < 2000000; i++) {
    uint8_t b[8];
    uint64_t t = 0;
    for (int j = 0; j < 8; j++) { b[j] = (uint8_t)(i < 256 ? (j == i % 8 ? 0xFF : i) : rnd()); t |= (uint64_t)b[j] << (8 * j); }
    uint64_t key40 = 0;
    for (int j = 3; j < 8; j++) key40 = (key40 << 8) | b[j];      // bytes 2..6 of the suffix, byte 2 on top
    CHECK(pk_key_of_text(t) == key40);
    CHECK(pk_key_of_text(t) == (pk_record(key40, 1u, 5u) >> PK_KEY_LO));      // what gen_key packs for the same suffix
    CHECK(pk_bytes01_of_text(t) == (((uint32_t)b[1] << 8) | b[2]));
    CHECK(pk_prev_of_text(t) == b[0]);
    CHECK(pk1_b2(pk1_of(pk_record(pk_key_of_text(t), 0u, 7u))) == b[3]);
  }
  if (fails) { fprintf(stderr, "bwt_pk1_check: %d checks failed\n", fails); return 1; }
  printf("bwt_pk1_check ok\n");
  return 0;
}
