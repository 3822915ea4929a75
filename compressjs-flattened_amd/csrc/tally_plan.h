// tally_plan.h -- the rule of the key tally (cjs_keys_tally) as tally.hip computes it in stages.  No HIP: the kernels
// and the host compiler read the same functions (tests/host/tally_plan_check.cc checks them against a naive std::map).
//   A GROUP is the set of records of keys[0 .. n) that are equal in all three fields (lk_same of line_key.h, the equality of the line
//   diff).  The all-ones record ("touches a bad block") belongs to no group.  A group has `first`, the lowest index of a member, and
//   `count`, the number of members.
//   The SORT that finds the groups is by the whole record: by hash, then by W1 = len << 32 | check, ties in input order.  The
//   all-ones record is the largest value of both words, so the bad records stand behind every group, and in a run of equal records
//   the head is the member of the lowest index: the group's `first`.  (Sorting by the hash alone is not enough: records of one hash
//   and different len / check may interleave, and the bases are public, so such input can be made.)
//   The FILTER keeps a group iff min_count <= count and (max_count == 0 or count <= max_count).
//   The ORDER of the kept groups is ascending in a 64-bit word: `first` (CJS_TALLY_BY_FIRST), or (~count & 0xFFFFFFFF) << 32 | first
//   (CJS_TALLY_BY_COUNT: descending count, ties by ascending first).  Both fit because n < 2^32, and both are total: no two groups
//   share a first.
// The order of `sort` itself, by content, is not here but in sort_plan.h: keys do not order as lines do.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <vector>
#include "cjs_hip.h"
#include "line_key.h"

#if defined(__HIPCC__)
#define TL_FN __host__ __device__ __forceinline__
#else
#define TL_FN inline
#endif

namespace cjs {

constexpr uint64_t TL_MAX_KEYS = 0xFFFFFFFEull;      // the sorter's indices are 32 bits

// the second sort word of a record (the first is its hash)
TL_FN uint64_t tl_w1(const cjs_bz_linekey& k) { return (uint64_t)k.len << 32 | k.check; }
// all three fields equal (the bad record included: the callers keep it apart)
TL_FN bool tl_equal(const cjs_bz_linekey& a, const cjs_bz_linekey& b) { return a.hash == b.hash && a.len == b.len && a.check == b.check; }
// a stands in front of b in the sort by the whole record
TL_FN bool tl_less(const cjs_bz_linekey& a, const cjs_bz_linekey& b) { return a.hash != b.hash ? a.hash < b.hash : tl_w1(a) < tl_w1(b); }
TL_FN bool tl_kept(uint64_t count, uint64_t min_count, uint64_t max_count) { return count >= min_count && (max_count == 0 || count <= max_count); }
// first, count < 2^32
TL_FN uint64_t tl_order_word(uint32_t order, uint64_t first, uint64_t count) {
  return order == CJS_TALLY_BY_COUNT ? ((~count & 0xFFFFFFFFull) << 32 | first) : first;
}
// The bits of the order word that can differ between two groups when no count is above max_count: the radix passes of the order
// sort cover [0, tl_order_bits) only (the digits above are equal in every word, and a stable pass over equal digits moves nothing).
inline int tl_order_bits(uint32_t order, uint64_t max_count) {
  if (order != CJS_TALLY_BY_COUNT) return 32;
  int b = 0;
  while (b < 32 && (max_count >> b)) b++;
  return 32 + ((b + 7) & ~7);
}
// the argument errors that every form of the call refuses alike (the pointers are the caller's to check)
inline bool tl_args_ok(uint32_t order, uint64_t min_count, uint64_t max_count) {
  return (order == CJS_TALLY_BY_FIRST || order == CJS_TALLY_BY_COUNT) && (max_count == 0 || max_count >= min_count);
}

// The stream tally keys a tail line that is not empty as if it ended in a newline: its open fragment, which the host join holds in
// full, joined with the one-byte fragment of "\n".
TL_FN LkFrag tl_join_newline(const LkFrag& open, const LkBases& B) { return lk_join(open, LkFrag{0x0A + 1, 0x0A + 1, 1}, B); }

// The rule restated with std::stable_sort (behind cjs_stage_keys_tally): out gets the first min(cap, n_groups) groups.
inline int tl_tally_host(const cjs_bz_linekey* keys, size_t n, uint32_t order, uint64_t min_count, uint64_t max_count, cjs_bz_tally* out, size_t cap,
                         cjs_tally_info* info) {
  if (!info || (!keys && n) || (!out && cap) || !tl_args_ok(order, min_count, max_count)) return CJS_E_INVALID_ARG;
  *info = cjs_tally_info{(uint64_t)n, 0, 0, 0, 0};
  if ((uint64_t)n > TL_MAX_KEYS) return CJS_E_UNSUPPORTED;
  std::vector<uint32_t> perm;
  perm.reserve(n);
  for (size_t i = 0; i < n; i++) { if (lk_is_bad(keys[i])) info->n_bad++; else perm.push_back((uint32_t)i); }
  std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return tl_less(keys[a], keys[b]); });
  std::vector<cjs_bz_tally> kept;
  for (size_t i = 0; i < perm.size();) {
    size_t j = i + 1;
    while (j < perm.size() && tl_equal(keys[perm[i]], keys[perm[j]])) j++;
    const uint64_t count = j - i;
    info->n_distinct++;
    info->max_count = std::max(info->max_count, count);
    if (tl_kept(count, min_count, max_count)) kept.push_back(cjs_bz_tally{keys[perm[i]], perm[i], count});
    i = j;
  }
  info->n_groups = kept.size();
  std::stable_sort(kept.begin(), kept.end(), [&](const cjs_bz_tally& a, const cjs_bz_tally& b) {
    return tl_order_word(order, a.first, a.count) < tl_order_word(order, b.first, b.count);
  });
  for (size_t i = 0; i < kept.size() && i < cap; i++) out[i] = kept[i];
  return 0;
}

}  // namespace cjs
