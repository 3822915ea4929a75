// bwt_rules.h — the rules that the suffix-sort kernels (bwt_round1.hip, bwt_tile_sort.hip, bwt_defer.hip, bwt_regroup.hip), the
// key source of radix.hpp and the round loop of bwt.hip must agree on, each once: the record layouts, the key arithmetic of round
// 1, the stepping of the rounds, the geometry and the ownership rule of the tile sorters' windows, and the large-group test.  No
// HIP: plain constexpr functions that the kernels and the host compiler read alike (tests/host/bwt_rules_check.cc walks every
// window of random group sequences with them, against a serial model).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace cjs {

constexpr int bits_for(uint64_t x) { int b = 0; while (x) { b++; x >>= 1; } return b; }      // bits needed to write x

// ---- limits.  Positions inside a block and ranks take RANK_BITS bits: a rank key is rank + 1 (0 = past the end, sentinel form),
// so a block holds at most 2^20 - 2 suffixes; slot numbers are 32 bits wide with room for a window past the last slot.
constexpr int RANK_BITS = 20;
constexpr uint32_t RANK_MASK = (1u << RANK_BITS) - 1u;
constexpr uint32_t BWT_MAX_STRIDE = (1u << RANK_BITS) - 2u;
constexpr uint64_t BWT_MAX_SLOTS = 0xFFFFF000ull;
constexpr bool bwt_admits(uint64_t slots, uint32_t stride) { return slots < BWT_MAX_SLOTS && stride <= BWT_MAX_STRIDE; }

// ---- record layouts
// packed records (cyclic round 1): ONE u64 per suffix = 5 bytes (bits 63..24) | block parity (bit 20) | position in the block
// (bits 19..0): a radix pass moves 8 B per suffix each way instead of 12, and there is no value array.  The first phase sorts by
// bytes 2..6 of the suffix (packed == 2, the only packed form)
constexpr int PK_SHIFT = RANK_BITS, PK_KEY_LO = 24;
constexpr uint32_t PK_POS_MASK = (1u << PK_SHIFT) - 1u;
constexpr uint64_t pk_record(uint64_t bytes2to6, uint32_t parity, uint32_t pos) {
  return ((bytes2to6 & 0xFFFFFFFFFFull) << PK_KEY_LO) | ((uint64_t)(parity & 1u) << PK_SHIFT) | (uint64_t)pos;
}
constexpr uint32_t pk_pos(uint64_t rec) { return (uint32_t)rec & PK_POS_MASK; }      // of every packed layout, and of val[]
// narrow records of the last phase-1 passes: ONE u32 per suffix = byte 2 (bits 27..20) | position (19..0).  An LSD pass only needs
// the digits that are still to come: behind the pass on byte 4 that is byte 3 (it rides in dig[]) and byte 2.  No parity bit:
// tiles never straddle a block, and whoever compares neighbours (bwt_phase2_records) stops at the block start by the slot number
constexpr int PK1_B2_SHIFT = PK_SHIFT;
constexpr uint32_t pk1_record(uint32_t b2, uint32_t pos) { return ((b2 & 0xFFu) << PK1_B2_SHIFT) | (pos & PK_POS_MASK); }
constexpr uint32_t pk1_of(uint64_t rec) { return pk1_record((uint32_t)(rec >> 56), pk_pos(rec)); }      // of a pk_record
constexpr uint32_t pk1_b2(uint32_t rec) { return rec >> PK1_B2_SHIFT; }
// the 40-bit class key of phase 1 (bytes 2..6, byte 2 on top) and the fields of the phase-2 record out of the eight text bytes
// around a suffix, byte j of `t` = text[position - 1 + j] (cyclic)
constexpr uint64_t pk_key_of_text(uint64_t t) { return ((t >> 24 & 0xFFu) << 32) | __builtin_bswap32((uint32_t)(t >> 32)); }
constexpr uint32_t pk_bytes01_of_text(uint64_t t) { return (uint32_t)((t >> 8 & 0xFFu) << 8 | (t >> 16 & 0xFFu)); }
constexpr uint32_t pk_prev_of_text(uint64_t t) { return (uint32_t)t & 0xFFu; }
// records of the two-phase sort after bwt_phase2_records: byte0 . byte1 (63..48) | rank of the class of bytes 2..6 (47..28) | the byte IN
// FRONT of the suffix (27..20) | position (19..0).  The group key is key >> PK2_GSHIFT; block boundaries are taken from the slot
// number (no parity bit).  The byte in front is what the BWT emits for the suffix: it rides along (later in the top byte of val[])
// so that the regroup kernels write BWT bytes without gathering them from the text.
constexpr int PK2_GSHIFT = 28, PK2_PREV_SHIFT = 20, VAL_PREV_SHIFT = 24;
constexpr uint64_t pk2_record(uint32_t bytes01, uint32_t r1, uint32_t prev, uint32_t pos) {
  return ((uint64_t)(bytes01 & 0xFFFFu) << 48) | ((uint64_t)r1 << PK2_GSHIFT) | ((uint64_t)prev << PK2_PREV_SHIFT) | (uint64_t)(pos & PK_POS_MASK);
}
constexpr uint32_t pk2_prev(uint32_t rec_lo) { return (rec_lo >> PK2_PREV_SHIFT) & 0xFFu; }
// val[] of the rounds >= 2: the position, and (cyclic, packed round 1) the byte in front of the suffix on top
constexpr uint32_t val_carrying(uint32_t pos, uint32_t prev) { return pos | (prev << VAL_PREV_SHIFT); }
constexpr uint32_t val_prev(uint32_t v) { return v >> VAL_PREV_SHIFT; }
// key of a round >= 2: group ordinal | rank key of the suffix h further on.  The keys that the tile sorters leave for the deferral
// kernels carry the slot's head bit (1 = starts a group) as the ordinal: bwt_defer_gather numbers the deferred groups from them
constexpr uint64_t round_key(uint32_t ordinal, uint32_t rank_key) { return ((uint64_t)ordinal << RANK_BITS) | rank_key; }
constexpr uint64_t round_key_ordinal(uint64_t k) { return k >> RANK_BITS; }
constexpr uint32_t round_key_rank(uint64_t k) { return (uint32_t)k & RANK_MASK; }
// flag byte of a slot behind the sort of a round >= 2
constexpr uint32_t HF_NEW = 1u, HF_OLD = 2u;     // head of the new grouping / of the previous round's grouping
constexpr uint8_t hf_byte(bool new_head, bool old_head) { return (uint8_t)((new_head ? HF_NEW : 0u) | (old_head ? HF_OLD : 0u)); }
// ... from a sorted (x << RANK_BITS | rank key) and the one in front of it, 64 or 32 bits wide
template <typename K> constexpr uint8_t hf_of_sorted(K k, K prev) { return (uint8_t)((k != prev ? HF_NEW : 0u) | ((k >> RANK_BITS) != (prev >> RANK_BITS) ? HF_OLD : 0u)); }
// bit `bit` of each of the 4 flag bytes in a word -> 4-bit mask (byte j -> bit j): bits 0, 8, 16, 24 of x land on bits 24..27 of
// x * 0x01020408 (no two partial products meet)
constexpr uint32_t hf_bits4(uint32_t word, int bit) { return ((((word >> bit) & 0x01010101u) * 0x01020408u) >> 24) & 15u; }
// composites of the tile sorters.  Counting / bitonic: head slot (63..52) | rank key (51..32) | suffix (31..0), slots that are not
// owned carry their own slot and the largest rank key; LDS radix: head slot (31..20) | rank key, others (own slot << 20)
constexpr uint64_t ts64_owned(uint32_t head_slot, uint32_t rank_key, uint32_t suffix) { return ((uint64_t)head_slot << 52) | ((uint64_t)rank_key << 32) | suffix; }
constexpr uint64_t ts64_other(uint32_t slot) { return ((uint64_t)slot << 52) | ((uint64_t)RANK_MASK << 32); }
constexpr uint32_t ts64_count_word(uint64_t e, uint32_t slot) { return ((uint32_t)(e >> 32) << 12) | slot; }      // rank key (31..12) | slot: the head slot falls off the top
constexpr uint32_t ts32_owned(uint32_t head_slot, uint32_t rank_key) { return (head_slot << RANK_BITS) | rank_key; }
constexpr uint32_t ts32_other(uint32_t slot) { return slot << RANK_BITS; }

// ---- round 1: the keys (block id | [VarGeom: hole bit] | nsym symbols), 8-bit symbols cyclic, 9-bit sentinel.  Segmented sorts
// keep the block id out of the key.  VarGeom: a hole's symbols are its position, which must fit them.
struct Round1Keys { int blk_bits, nsym, bits; };
constexpr int sym_bits_of(bool cyclic) { return cyclic ? 8 : 9; }
constexpr Round1Keys round1_keys(uint32_t nb, bool cyclic, bool segmented, bool var) {
  const int sym_bits = sym_bits_of(cyclic);
  const int blk_bits = bits_for(nb - 1) + (var ? 1 : 0);           // (VarGeom: + the hole bit)
  const int nsym = segmented || (64 - blk_bits) / sym_bits > 7 ? 7 : (64 - blk_bits) / sym_bits;
  return {blk_bits, nsym, nsym * sym_bits + (segmented ? 0 : blk_bits)};
}
constexpr int r1_block_shift(bool cyclic, int nsym) { return (cyclic ? 8 : 9) * nsym; }             // Geom: the block id sits on the symbols
constexpr int r1_hole_bit(int nsym) { return 8 * nsym; }                                            // VarGeom (cyclic): the hole bit, the block id above it
constexpr bool var_geom_admits(int nsym) { return nsym >= 3; }      // 24 symbol bits hold a position below 2^20, 16 do not

// ---- the rounds
// Slots of BwtWork::counters and of their pinned mirror h_counters.  bwt_scan_tiles writes the survivors, the groups and the
// large-group flag (it moves the flag to the mirror and clears it); the deferral scans of sort_round write the other two.
enum Counter { CN_SURVIVORS = 0, CN_GROUPS = 1, CN_DEFERRED = 2, CN_DEFERRED_GROUPS = 3, CN_LARGE_GROUP = 4 };
constexpr uint32_t next_depth(uint32_t h) { return h < (1u << 29) ? h * 2 : h; }
constexpr int round_key_bits(uint32_t ngroups) { return RANK_BITS + bits_for(ngroups ? ngroups - 1 : 0); }      // ordinals 0 .. ngroups-1 above the rank key

// ---- the tile sorters' windows.  A window owns the groups whose head lies in its nominal TS_NOM slots and loads TS_WIN slots
// (TS_MAXGRP of slack behind the nominal range, so every owned group is complete); TS_TINY: groups up to this size are ranked by
// counting; TS_GT: tile of the deferral kernels.
constexpr uint32_t TS_WIN = 4096, TS_MAXGRP = 1024, TS_NOM = TS_WIN - TS_MAXGRP, TS_TINY = 64, TS_GT = 2048;
constexpr uint32_t ts_windows(uint32_t A) { return (A + TS_NOM - 1) / TS_NOM; }
constexpr uint64_t ts_win_base(uint32_t win) { return (uint64_t)win * TS_NOM; }
constexpr uint32_t ts_win_len(uint64_t wb, uint32_t A) { return (uint32_t)((wb + TS_WIN < A ? wb + TS_WIN : A) - wb); }
// the tile sorters take the round (small remainders: whole-array radix passes on keys that bwt_gather_keys writes first)
constexpr bool tile_sorted_round(uint32_t A) { return A >= 2 * TS_WIN; }
// Which tile sorter: the LDS radix version costs the same whatever the groups look like (18 ps per suffix), the counting /
// bitonic version is cheaper once the groups are tiny (round 2 of the bench text, 7.7 suffixes per group: 1.51 vs 1.82 ms;
// round 3, 3.5 per group: 0.67 vs 0.64 ms; later rounds up to 2x in favour of counting)
constexpr bool radix_tile_sorter(uint32_t A, uint32_t ngroups) { return ngroups && A / ngroups >= 5; }
// the deferred groups are sorted apart in the spare halves of the workspace: no room for more than half of it
constexpr bool deferred_overflow(size_t D, size_t cap) { return D > cap / 2; }

// Heads of a window as 64 mask words (bit l of word i = slot 64 * i + l starts a group).  For a slot: the head of its group is
// the last head at or before it, in its word or (wlast) in the words in front, -1 = in front of the window; the next head is the
// first one behind it, in its word or (wnext) in the words behind, TS_WIN + 1 = none in the window.
constexpr int TS_NO_HEAD = -1, TS_NO_NEXT = (int)TS_WIN + 1;
constexpr uint64_t mask_le(int lane) { return lane == 63 ? ~0ull : ((2ull << lane) - 1ull); }
constexpr uint64_t mask_gt(int lane) { return lane == 63 ? 0ull : ~((2ull << lane) - 1ull); }
constexpr int word_last(uint64_t m, int word) { return m ? word * 64 + 63 - (int)__builtin_clzll(m) : TS_NO_HEAD; }
constexpr int word_first(uint64_t m, int word) { return m ? word * 64 + (int)__builtin_ctzll(m) : TS_NO_NEXT; }
constexpr int ts_head_of(uint64_t m, int word, int lane, int wlast) { return (m & mask_le(lane)) ? word_last(m & mask_le(lane), word) : wlast; }
constexpr int ts_next_of(uint64_t m, int word, int lane, int wnext) { return (m & mask_gt(lane)) ? word_first(m & mask_gt(lane), word) : wnext; }
// a next head past the L slots of the window: the array end closes the last group, anything else runs out of the window
constexpr int ts_close(int nx, uint32_t L, bool at_end) { return nx > (int)L ? (at_end ? (int)L : TS_NO_NEXT) : nx; }
// Ownership of a (valid) slot whose group is [hx, nx) in window slots, nx as the masks give it: small = the group is whole inside
// the window's L slots and has at most TS_MAXGRP members; owned = and its head lies in the nominal range, so THIS window sorts
// it (and clears its defer flags); medium = owned and too large for counting
struct TsOwn { bool small, owned, medium; };
constexpr TsOwn ts_classify(int hx, int nx, uint32_t L, bool at_end) {
  const int e = ts_close(nx, L, at_end);
  const bool small = hx >= 0 && e <= (int)L && (uint32_t)(e - hx) <= TS_MAXGRP;
  const bool owned = small && (uint32_t)hx < TS_NOM;
  return {small, owned, owned && (e - hx) > (int)TS_TINY};
}
// The group that runs into a window from the left, when the window's first slot is no head.  Thread t looks at the head bits of
// slots [4t, 4t + 4) of the TS_MAXGRP in front of the window (heads4: bit j = slot 4t + j starts a group): the index of the last
// head among its four, 0 = none.  The maximum over the threads is where that group starts, which leaves TS_MAXGRP - li_max of its
// members in front of the window (TS_MAXGRP: or more -- a head on index 0 and no head at all read the same, and both are too many
// for ts_prev_end).
constexpr uint32_t ts_li4(uint32_t t, uint32_t heads4) { return (heads4 & 15u) ? t * 4u + 31u - (uint32_t)__builtin_clz(heads4 & 15u) : 0u; }
// The same on group ordinals (the serial model of the host check numbers its groups): index + 1 of the last of the four ordinals
// that differs from the window's first ordinal g0.  With g0 the ordinal of a group that starts in front of the window, the two
// forms agree.
constexpr uint32_t ts_li4(uint32_t t, uint32_t q0, uint32_t q1, uint32_t q2, uint32_t q3, uint32_t g0) {
  return q3 != g0 ? t * 4u + 4u : q2 != g0 ? t * 4u + 3u : q1 != g0 ? t * 4u + 2u : q0 != g0 ? t * 4u + 1u : 0u;
}
// slots [0, result) of the window belong to a group that the window before owns.  m0 = first mask word of this window, wnext0 =
// first head behind that word
constexpr uint32_t ts_prev_end(uint64_t wb, uint32_t L, bool at_end, uint32_t li_max, uint64_t m0, int wnext0) {
  if (!wb || (m0 & 1ull)) return 0u;              // the first slot starts a group
  const uint32_t sb = TS_MAXGRP - li_max;         // members in front of the window (TS_MAXGRP: or more)
  const uint32_t fh = m0 ? (uint32_t)__builtin_ctzll(m0) : (uint32_t)wnext0;
  const uint32_t e = fh <= L ? fh : (at_end ? L : TS_WIN + 1u);
  return sb + e <= TS_MAXGRP ? e : 0u;
}
// Windows overlap, so every slot has ONE window that fetches its rank: the window that owns its group, else the window whose
// nominal range holds it -- unless the window before owns it
constexpr bool ts_fetches(bool valid, uint32_t x, uint32_t prev_end, bool owned) { return valid && x >= prev_end && (owned || x < TS_NOM); }

// ---- the large-group test of the regroup.  A group of more than TS_MAXGRP - 1 slots covers a whole aligned run of LG_RUN slots:
// when every such run below A holds a head, no group is too large for the tile sorters of the next round (the host then skips
// their deferral bookkeeping).  It also fires for smaller groups that happen to cover an aligned run behind their head: the
// smallest has LG_RUN + 1 slots.
// heads: bit j = piece j holds a head, `per` pieces to a run, piece 0 starts at slot `base` (a multiple of LG_RUN)
constexpr uint32_t LG_RUN = TS_MAXGRP / 2;
constexpr bool run_without_head(uint64_t heads, uint32_t per, uint64_t base, uint32_t A) {
  bool bad = false;
  for (uint32_t b = 0; b * per < 64u; b++)
    bad |= base + (uint64_t)(b + 1u) * LG_RUN <= A && ((heads >> (b * per)) & (per < 64u ? (1ull << per) - 1ull : ~0ull)) == 0;
  return bad;
}

}  // namespace cjs
