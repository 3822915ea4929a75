// huff_rules.h — the arithmetic of the entropy stage (Huffman tables, the block's bit layout, the stream frame, the workspace),
// each rule once.  No HIP: plain constexpr functions that the kernels of huff_tables.hip and huff_pack.hip, huff.h, stages.hip
// and the host compiler read alike (tests/host/huff_rules_check.cc checks them against the oracle).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "bz_frame.h"

#define CJS_RULE __attribute__((always_inline)) constexpr

namespace cjs {

// ---- constants
constexpr int MAXSYM = 258;              // symbols of a table: 256 byte ranks + RUNA/RUNB folded + EOB
constexpr int MAX_BITS = 20;             // longest code
constexpr int GSZ = 50;                  // symbols per selector group
constexpr int PD_GROUPS = 80;            // groups per data-packing tile (4000 symbols)
constexpr int MAXTAB = 6;                // tables per block
constexpr int WL_W = 264, FREQ_W = 260;  // row widths of the lengths / counts between the kernels of the chain (and in LDS)
constexpr int AS_GROUPS = 512;           // groups per step of assign_selectors
constexpr uint32_t HS_STEPS = 4;         // 512-group steps per workgroup of hs_assign
constexpr uint32_t HS_CNT = 131072;      // symbols per workgroup of hs_count
// per block: lens u8[6][258] and codes u32[6][258]; wl u8[6][264]; wfreq u32[6][260]
constexpr size_t lens_row_bytes() { return (size_t)MAXTAB * MAXSYM; }
constexpr size_t codes_row_elems() { return (size_t)MAXTAB * MAXSYM; }
constexpr size_t wl_row_bytes() { return (size_t)MAXTAB * WL_W; }
constexpr size_t wfreq_row_elems() { return (size_t)MAXTAB * FREQ_W; }

// ---- geometry
constexpr int huff_target(uint32_t npos) { return npos >= 2400 ? 6 : npos >= 1200 ? 5 : npos >= 600 ? 4 : npos >= 200 ? 3 : 2; }   // Bzip2:2150
template <typename T> constexpr T groups_for(T npos) { return (npos + GSZ - 1) / GSZ; }                    // selectors of npos symbols
constexpr uint32_t tiles_for_groups(uint32_t nsel) { return (nsel + PD_GROUPS - 1) / PD_GROUPS; }
// a block of up to `stride` bytes yields up to stride + 1 symbols; rows of selectors are padded to 64
constexpr size_t sel_stride_for(uint32_t stride) { return (groups_for((size_t)stride + 1) + 63) & ~(size_t)63; }
constexpr size_t tile_stride_for(size_t sel_stride) { return sel_stride / PD_GROUPS + 2; }
constexpr uint32_t hs_assign_grid(uint32_t max_stride) { return (uint32_t)((groups_for((size_t)max_stride + 1) + HS_STEPS * AS_GROUPS - 1) / (HS_STEPS * AS_GROUPS)); }
constexpr uint32_t hs_count_grid(uint32_t max_stride) { return (max_stride + 1 + HS_CNT - 1) / HS_CNT; }

// ---- the length-limited allocator (Bzip2:1085-1301), in place on the sorted frequencies a[0..len)
// a[] entries below the root are extended parent pointers p or p + len (p < len), so "% len" is one conditional subtract
CJS_RULE int ha_mod(int x, int len) { return x >= len ? x - len : x; }
CJS_RULE int ha_first(const int* a, int len, int i, int nodes_to_move) {          // Bzip2:1135-1156
  const int limit = i;
  int k = len - 2;
  while (i >= nodes_to_move && ha_mod(a[i], len) > limit) { k = i; i -= (limit - i + 1); }
  if (i < nodes_to_move - 1) i = nodes_to_move - 1;
  while (k > i + 1) {
    const int mid = (i + k) >> 1;
    if (ha_mod(a[mid], len) > limit) k = mid; else i = mid;
  }
  return k;
}
// pass 1 (one lane): extended parent pointers (Bzip2:1162-1186); false when len < 3 (lengths written, nothing left to do)
CJS_RULE bool ha_pass1(int* a, int len) {
  if (len == 2) { a[1] = 1; a[0] = 1; return false; }
  if (len == 1) { a[0] = 1; return false; }
  a[0] += a[1];
  // the two queue fronts live in registers two deep (H = a[head], Hn = a[head+1], T = a[top], Tn = a[top+1]), so the
  // LDS reads that refill them overlap the comparisons instead of sitting on the critical path
  int head = 0, top = 2;
  int H = a[0], Hn = 0;
  int T = top < len ? a[top] : 0, Tn = top + 1 < len ? a[top + 1] : 0;
  for (int tail = 1; tail < len - 1; tail++) {
    int w = 0;
    if (top >= len || H < T) { w = H; a[head++] = tail; H = Hn; if (head + 1 < tail) Hn = a[head + 1]; }
    else { w = T; top++; T = Tn; if (top + 1 < len) Tn = a[top + 1]; }
    if (top >= len || (head < tail && H < T)) { w += H; a[head++] = tail + len; H = Hn; if (head + 1 < tail) Hn = a[head + 1]; }
    else { w += T; top++; T = Tn; if (top + 1 < len) Tn = a[top + 1]; }
    a[tail] = w;
    if (head == tail) H = w; else if (head + 1 == tail) Hn = w;
  }
  return true;
}
// passes 2 and 3 over the array that pass 1 left; root0 = ha_mod(a[0], len).  first_of(limit, lo) = ha_first(a, len, limit, lo),
// fill(lo, hi, x): a[lo..hi] = x, peek(i) = a[i] as the array stands (fills included); between() runs once, after pass 2.
struct HaNoMark { constexpr void operator()() const {} };
template <typename First, typename Fill, typename Peek, typename Mark = HaNoMark>
CJS_RULE void ha_passes23(int len, int maxlen, int root0, First first_of, Fill fill, Peek peek, Mark between = Mark()) {
  // pass 2: nodes to relocate (Bzip2:1195-1204)
  int reloc = len - 2;
  for (int depth = 1; depth < maxlen - 1 && reloc > 1; depth++) reloc = first_of(reloc - 1, 0);
  between();
  // pass 3
  if (root0 >= reloc) {                                                            // Bzip2:1211-1226
    int first = len - 2, next = len - 1;
    for (int depth = 1, avail = 2; avail > 0; depth++) {
      const int last = first;
      first = first_of(last - 1, 0);
      const int cnt = avail - (last - first);
      if (cnt > 0) { fill(next - cnt + 1, next, depth); next -= cnt; }
      avail = (last - first) << 1;
    }
  } else {                                                                          // Bzip2:1235-1264
    const unsigned rm1 = (unsigned)(reloc - 1);
    const int insert_depth = maxlen - (rm1 ? 32 - __builtin_clz(rm1) : 0);      // Util.fls
    int first = len - 2, next = len - 1;
    int depth = insert_depth == 1 ? 2 : 1;
    int left = insert_depth == 1 ? reloc - 2 : reloc;
    for (int avail = depth << 1; avail > 0; depth++) {
      const int last = first;
      first = first <= reloc ? first : first_of(last - 1, reloc);
      int offset = 0;
      if (depth >= insert_depth) { offset = 1 << (depth - insert_depth); if (left < offset) offset = left; }
      else if (depth == insert_depth - 1) {
        offset = 1;
        if (peek(first) == last) first++;
      }
      const int cnt = avail - (last - first + offset);
      if (cnt > 0) { fill(next - cnt + 1, next, depth); next -= cnt; }
      left -= offset;
      avail = (last - first + offset) << 1;
    }
  }
}
// the allocator's input order: symbols by (frequency, index) ascending, as one key per symbol (Bzip2:1881-1883)
constexpr uint32_t rank_key(uint32_t freq, uint32_t i) { return (freq << 9) | i; }

// ---- canonical codes (Bzip2:1896-1916): code = first code of the length + rank among the smaller symbols of the same length
CJS_RULE void canon_first_codes(const uint32_t* lhist /* [MAX_BITS + 1] symbols per length */, uint32_t* fc) {
  uint32_t code = 0;
  for (int l = 1; l <= MAX_BITS; l++) { code <<= 1; fc[l] = code; code += lhist[l]; }
}
CJS_RULE uint32_t canon_rank(const uint8_t* lens, int s) {
  uint32_t r = 0;
  for (int k = 0; k < s; k++) r += lens[k] == lens[s];
  return r;
}
constexpr void canonical_codes(const uint8_t* lens, int n, uint32_t* codes) {
  uint32_t lhist[MAX_BITS + 1] = {}, fc[MAX_BITS + 1] = {};
  for (int s = 0; s < n; s++) lhist[lens[s]]++;
  canon_first_codes(lhist, fc);
  for (int s = 0; s < n; s++) codes[s] = fc[lens[s]] + canon_rank(lens, s);
}

// ---- the block's bit layout: what the packer emits, item by item; the accounting adds the items' nbits
struct BitItem { uint64_t val; uint32_t nbits; };
constexpr uint32_t HEADER_ITEMS = 22;    // (the last one is empty)
// header: magic(48) crc(32) rand(1)+pidx(24) coarse(16) fine(16 each, of the ranges in use) ngroups(3)+nsel(15)
CJS_RULE BitItem header_item(uint32_t i, uint32_t crc, uint32_t pidx, uint32_t coarse, const uint32_t* fine, uint32_t ng, uint32_t nsel) {
  if (i == 0) return BitItem{MAGIC_BLOCK, 48};
  if (i == 1) return BitItem{crc, 32};
  if (i == 2) return BitItem{pidx & 0xFFFFFFu, 25};
  if (i == 3) return BitItem{coarse, 16};
  if (i < 20) { const uint32_t r = i - 4; return (coarse & (0x8000u >> r)) ? BitItem{fine[r], 16} : BitItem{0, 0}; }
  if (i == 20) return BitItem{((uint64_t)ng << 15) | nsel, 18};
  return BitItem{0, 0};
}
// selector with MTF position j: j ones and a zero (Bzip2:2171-2182)
CJS_RULE BitItem selector_item(uint32_t j) { return BitItem{((1ull << j) - 1ull) << 1, j + 1}; }
// a table entry (Bzip2:1926-1947): '10' per step up or '11' per step down from the previous length, then '0'; the first entry
// of a table has the 5-bit start length in front and no steps (the caller passes prev = cur)
CJS_RULE BitItem table_item(uint32_t cur, uint32_t prev, bool first) {
  const uint32_t d = cur > prev ? cur - prev : prev - cur;
  const uint64_t pat = cur > prev ? 2ull : 3ull;
  uint64_t v = 0;
  for (uint32_t k = 0; k < d; k++) v = (v << 2) | pat;
  v <<= 1;
  if (first) v |= (uint64_t)cur << 1;
  return BitItem{v, 2 * d + 1 + (first ? 5u : 0u)};
}
// bits of a block: magic + CRC, rand + pidx, coarse map, a fine map per range in use, ngroups + nsel, selectors, tables, data
constexpr uint32_t block_bits(uint32_t nranges, uint32_t sel_bits, uint32_t tab_bits, uint32_t data_bits) {
  return 48u + 32u + 25u + 16u + 16u * nranges + 18u + sel_bits + tab_bits + data_bits;
}

// ---- the stream frame: 'BZh<level>' in front; end-of-stream magic (48) and stream CRC (32) behind
constexpr uint32_t STREAM_HEADER_BITS = 32, STREAM_TRAILER_BITS = 48 + 32;
constexpr uint64_t framed_bits(uint64_t bitlen) { return STREAM_HEADER_BITS + bitlen + STREAM_TRAILER_BITS; }
// capacity: the packers store whole 32-bit words and OR boundary words, so a stream that ends at bit `end` (trailer not
// counted) needs 8 bytes of room behind its last byte; 16 bytes behind it are zeroed, as far as the buffer goes
constexpr uint64_t stream_bytes(uint64_t end, uint64_t trailer_bits) { return (end + trailer_bits + 7) / 8; }
constexpr bool stream_too_small(uint64_t end, uint64_t trailer_bits, uint64_t cap_bytes) { return stream_bytes(end, trailer_bits) + 8 > cap_bytes; }
constexpr uint64_t stream_zeroed_bytes(uint64_t end, uint64_t trailer_bits, uint64_t cap_bytes) {
  return stream_bytes(end, trailer_bits) + 16 > cap_bytes ? cap_bytes : stream_bytes(end, trailer_bits) + 16;
}

// ---- one bit-splitting rule: the nbits (<= 64) low bits of val, MSB first, from stream bit `bit` on, as the pieces that fall into
// the stream's big-endian 32-bit words: put(word index, the piece at its place in the word)
template <typename Put>
CJS_RULE void split_bits(uint64_t bit, uint64_t val, uint32_t nbits, Put put) {
  uint64_t w = bit >> 5;
  uint32_t o = (uint32_t)(bit & 31);
  uint32_t left = nbits;
  while (left) {
    const uint32_t room = 32 - o, take = left < room ? left : room;
    const uint32_t chunk = (uint32_t)((val >> (left - take)) & (take == 32 ? 0xFFFFFFFFull : ((1ull << take) - 1ull)));
    put(w, chunk << (room - take));
    left -= take; o = 0; w++;
  }
}

// ---- workspace: element counts of the thirteen sub-buffers of HuffWork, in carve order, each carved at a 256-byte boundary
enum HuffBuf { HB_SEL, HB_SELJ, HB_BCOST, HB_LENS, HB_CODES, HB_NGROUPS, HB_BITLEN, HB_BITOFF, HB_SCALARS, HB_DATABITS, HB_TILEOFF, HB_WL, HB_WFREQ, HB_COUNT };
constexpr size_t HUFF_ELEM_BYTES[HB_COUNT] = {1, 1, 2, 1, 4, 4, 4, 8, 8, 4, 4, 1, 4};
struct HuffLayout { size_t sel_stride, tile_stride, n[HB_COUNT]; };
constexpr HuffLayout huff_layout(size_t max_blocks, uint32_t stride) {
  const size_t ss = sel_stride_for(stride), ts = tile_stride_for(ss);
  return {ss, ts, {max_blocks * ss, max_blocks * ss, max_blocks * ss, max_blocks * lens_row_bytes(), max_blocks * codes_row_elems(),
                   max_blocks, max_blocks, max_blocks + 1, 8, max_blocks, max_blocks * ts, max_blocks * wl_row_bytes(), max_blocks * wfreq_row_elems()}};
}
constexpr size_t huff_layout_bytes(const HuffLayout& L) {
  size_t b = 0;
  for (int i = 0; i < HB_COUNT; i++) b += (L.n[i] * HUFF_ELEM_BYTES[i] + 255) & ~(size_t)255;
  return b + 4096;
}

}  // namespace cjs
