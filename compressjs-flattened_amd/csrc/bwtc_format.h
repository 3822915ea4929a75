// bwtc_format.h — what the two sides of the BWTC stream and the model kernels share: the coder step word the kernels write and
// the host coder reads, and the format's small arithmetic (bit lengths, the use-tree's node sizes).  No HIP in here
// (tests/host/bwtc_host_check.cc compiles it with the host compiler).
#pragma once
#include <stdint.h>

namespace cjs {

// A coder step is one call of RangeCoder.encodeFreq / encodeShift (J/BWTC_joined_.js:92-113): sy | lt << 16 | tot << 32, with the
// shift in tot's place when STEP_SHIFT_FLAG is set.
constexpr uint64_t STEP_SHIFT_FLAG = 1ull << 63;   // step is encodeShift(sy, lt, shift) instead of encodeFreq
struct Step { uint32_t sy, lt, tot; };
inline Step unpack(uint64_t st) { return {(uint32_t)(st & 0xFFFF), (uint32_t)((st >> 16) & 0xFFFF), (uint32_t)((st >> 32) & 0x1FFFF)}; }
// a step the reference's models could make: sy >= 1, lt + sy <= tot < 2^17, or a shift of 1..16 with lt + sy <= 1 << shift
inline bool step_valid(uint64_t st) {
  const Step s = unpack(st);
  if (((st >> 49) & 0x3FFF) || s.sy < 1) return false;
  if (st & STEP_SHIFT_FLAG) return s.tot >= 1 && s.tot <= 16 && s.lt + s.sy <= (1u << s.tot);
  return s.lt + s.sy <= s.tot;
}

inline int fls32(uint32_t v) { int r = 0; while (v) { r++; v >>= 1; } return r; }
// LogDistanceModel (:1241-1261): bits of the length prefix of a distance below block_size
inline int lgbits(int block_size) { return fls32((uint32_t)(1 + fls32((uint32_t)block_size - 1)) - 1); }
// use-tree (:1744-1765, :1859-1874): leaves under one child of the parent of heap node i (1..511); the parent holds 0..2 * full
inline int use_tree_full(int i) { return 1 << (9 - fls32((uint32_t)i)); }

}  // namespace cjs
