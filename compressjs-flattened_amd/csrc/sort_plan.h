// sort_plan.h -- the rule of the line sort (cjs_text_sort, cjs_bzip2_sort) as sort.hip computes it in rounds.  No HIP:
// the kernels and the host compiler read the same functions (tests/host/sort_plan_check.cc checks them against std::stable_sort
// with memcmp).
//   A LINE of a text is the bytes between newlines, without the newline.  A tail that is not empty is a line, an empty tail is none
//   (the tail rule of the cut and the tally).  Lines are numbered from 0.
//   The ORDER is bytewise as memcmp, a proper prefix before the longer line (LC_ALL=C sort, Python's order of bytes); equal lines go
//   by ascending line number.  CJS_SORT_REVERSE: descending content, equal lines still by ascending line number.  Both are total.
//   The ROUND WORD of a line at depth d = 7 r: (bytes [d, d + 7) of the line, big-endian, zero-padded) << 8 | min(7, max(0, len - d)).
//   The low byte makes padding sort below a real 0x00 ("ab" < "ab\0" < "ab\0\0"); a line whose low byte is below 7 has ended, and two
//   lines with equal words whose low byte is below 7 are equal in full.
//   ROUND r sorts every active group by the word at depth 7 r, stably, and splits it where neighbours differ.  Round 0 has one group
//   of all lines, in line order.  A group is DONE when it has one member or its word's low byte is below 7, else ACTIVE; a group
//   holds a contiguous run of slots of the final order and a round only permutes inside it.  The rounds run = 1 + the largest
//   floor(common prefix / 7) over neighbours of the final order <= (longest line + 8) / 7.
//   After the last round the groups are the runs of equal lines, each led by its lowest line number (every sort is stable).
//   CJS_SORT_UNIQUE emits each group's first line (and its size as the count), else every line (count 1).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <vector>
#include "cjs_hip.h"

#if defined(__HIPCC__)
#define SL_FN __host__ __device__ __forceinline__
#else
#define SL_FN inline
#endif

namespace cjs {

constexpr uint64_t SL_MAX_BYTES = 0xFFFFFFFEull;      // starts and lengths are 32 bits (and start[lines] may be n + 1)
constexpr uint64_t SL_MAX_LINES = 0xFFFFFFFEull;      // the sorter's values are 32 bits
constexpr uint32_t SL_TEXT_TILE = 4096;               // text bytes of a workgroup of sl_count / sl_starts: 256 threads x 16
constexpr uint32_t SL_TILE = 1024;                    // slots of a workgroup of the flag and rank kernels: 256 threads x 4
constexpr uint32_t SL_OUT_TILE = 4096;                // output bytes of a workgroup of sl_gather

// the round word of the line p[0 .. len) at depth d (d may be beyond the line)
SL_FN uint64_t sl_word(const uint8_t* p, uint64_t len, uint64_t d) {
  const uint64_t left = len > d ? len - d : 0, k = left < 7 ? left : 7;
  uint64_t w = 0;
  for (uint64_t i = 0; i < 7; i++) w = w << 8 | (i < k ? p[d + i] : 0);
  return w << 8 | k;
}
SL_FN bool sl_word_ended(uint64_t w) { return (w & 0xFF) < 7; }
// the most rounds a text whose longest line has `longest` bytes can take
SL_FN uint64_t sl_max_rounds(uint64_t longest) { return (longest + 8) / 7; }
inline bool sl_flags_ok(uint32_t flags) { return (flags & ~(uint32_t)(CJS_SORT_REVERSE | CJS_SORT_UNIQUE)) == 0; }
// the argument errors that every form of the primitive refuses alike (text_out / text_n: both or neither)
inline int sl_args(const void* text, uint64_t n, uint32_t flags, const void* lines_out, uint64_t cap, bool text_ptr, bool text_n_ptr, const void* info) {
  if (!info || (!text && n) || (!lines_out && cap) || text_ptr != text_n_ptr || !sl_flags_ok(flags)) return CJS_E_INVALID_ARG;
  return 0;
}
inline void sl_info_clear(cjs_bz_sort_info* info) { *info = cjs_bz_sort_info{0, 0, 0, 0, 0, 0, 0, ~0ull}; }

// Device bytes of a sort of `lines` lines over `text_bytes` of text beyond the text, the outputs and the sorter's histograms
// (RadixWork): 8 per text tile of 4 KiB, and per line
//   4 start, 4 order, 1 head flag, 1 round flag, 2 x 8 sort keys, 8 kept words, 2 x 4 sort values, 2 x 4 group keys,
//   2 x 3 x 4 the active set (slot, line, group) of this round and the next, 4 group positions, 4 emitted lines, 8 text offsets
// = 90, and two counts per tile of 1024 lines.  Every array is padded to 256 bytes.
inline size_t sl_pad(size_t x) { return (x + 255) & ~(size_t)255; }
inline size_t sl_text_tiles(size_t text_bytes) { return (text_bytes + 15) / SL_TEXT_TILE + 1; }      // (+ 15: tiles start at an aligned address)
inline size_t sl_tiles(size_t lines) { return (lines + SL_TILE - 1) / SL_TILE; }
inline size_t sl_count_bytes(size_t text_bytes) { return sl_pad(8 * (sl_text_tiles(text_bytes) + 1)) + sl_pad(8 * 8); }
inline size_t sl_lines_bytes(size_t lines) {
  const size_t L = lines ? lines : 1;
  return 2 * sl_pad(8 * (sl_tiles(L) + 1)) + sl_pad(8 * 8) + sl_pad(4 * (L + 1)) + 13 * sl_pad(4 * L) + 2 * sl_pad(L) + 3 * sl_pad(8 * L) + sl_pad(8 * (L + 1));
}
inline size_t sl_work_bytes(size_t lines, size_t text_bytes) { return sl_count_bytes(text_bytes) + sl_lines_bytes(lines); }

struct SlLine { const uint8_t* p; uint64_t len; };
// the lines of text[0 .. n) by the tail rule
inline std::vector<SlLine> sl_lines_host(const uint8_t* text, size_t n) {
  std::vector<SlLine> v;
  size_t s = 0;
  for (size_t i = 0; i < n; i++) if (text[i] == 0x0A) { v.push_back(SlLine{text + s, i - s}); s = i + 1; }
  if (s < n) v.push_back(SlLine{text + s, n - s});
  return v;
}

// The rule on the host, round by round (behind cjs_stage_text_sort): lines_out / counts_out get the first min(cap, n_out) entries.
inline int sl_sort_host(const uint8_t* text, size_t n, uint32_t flags, uint64_t* lines_out, uint64_t* counts_out, size_t cap, cjs_bz_sort_info* info) {
  if (int rc = sl_args(text, n, flags, lines_out, cap, false, false, info)) return rc;
  sl_info_clear(info);
  if ((uint64_t)n > SL_MAX_BYTES) return CJS_E_UNSUPPORTED;
  const std::vector<SlLine> ln = sl_lines_host(text, n);
  const size_t L = ln.size();
  info->n_lines = L;
  std::vector<uint32_t> order(L);
  for (size_t i = 0; i < L; i++) order[i] = (uint32_t)i;
  std::vector<uint8_t> head(L, 0);
  struct Run { size_t lo, hi; };
  std::vector<Run> active, next;
  if (L) { active.push_back(Run{0, L}); head[0] = 1; }
  std::vector<std::pair<uint64_t, uint32_t>> rec;
  uint64_t rounds = 0;
  for (; !active.empty(); rounds++) {
    const uint64_t d = 7 * rounds;
    next.clear();
    for (const Run& g : active) {
      rec.clear();
      for (size_t s = g.lo; s < g.hi; s++) rec.push_back({sl_word(ln[order[s]].p, ln[order[s]].len, d), order[s]});
      std::stable_sort(rec.begin(), rec.end(), [](const std::pair<uint64_t, uint32_t>& a, const std::pair<uint64_t, uint32_t>& b) { return a.first < b.first; });
      for (size_t k = 0; k < rec.size();) {
        size_t e = k + 1;
        while (e < rec.size() && rec[e].first == rec[k].first) e++;
        head[g.lo + k] = 1;
        if (e - k > 1 && !sl_word_ended(rec[k].first)) next.push_back(Run{g.lo + k, g.lo + e});
        k = e;
      }
      for (size_t k = 0; k < rec.size(); k++) order[g.lo + k] = rec[k].second;
    }
    active.swap(next);
  }
  info->rounds = rounds;
  std::vector<size_t> gpos;
  for (size_t s = 0; s < L; s++) if (head[s]) gpos.push_back(s);
  const size_t nd = gpos.size();
  gpos.push_back(L);
  info->n_distinct = nd;
  const bool rev = flags & CJS_SORT_REVERSE, uniq = flags & CJS_SORT_UNIQUE;
  info->n_out = uniq ? nd : L;
  size_t at = 0;
  for (size_t k = 0; k < nd; k++) {
    const size_t g = rev ? nd - 1 - k : k, lo = gpos[g], hi = gpos[g + 1];
    for (size_t s = lo; s < (uniq ? lo + 1 : hi); s++, at++) {
      info->text_bytes += ln[order[s]].len + 1;
      if (at < cap) { lines_out[at] = order[s]; if (counts_out) counts_out[at] = uniq ? hi - lo : 1; }
    }
  }
  return 0;
}

}  // namespace cjs
