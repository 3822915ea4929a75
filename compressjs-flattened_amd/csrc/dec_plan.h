// dec_plan.h — host arithmetic of the Bzip2 decode phases: the row layout and row batches of phase A (dec_blocks.hip), a streaming
// step's row limit, and the inverse-BWT batches of phases B and C with the slot plan of one (dec_ibwt.hip).  No HIP in here
// (tests/host/plan_check.cc compiles it with the host compiler); what belongs to a kernel's file -- its tile, its row record --
// comes in as an argument.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <vector>

namespace cjs {

// One splitter every SPL slots of the LF vector.  A walk ends where it lands on a splitter slot -- a 1-in-SPL chance per step --,
// so the segments are geometric and the walk kernels last as long as the LONGEST of a block's segments, ~SPL x ln(n / SPL) steps
// of dependent loads (1,100 at 128, 610 at 64): halving SPL halves them; the splitter chain of a block (14,064 nodes at level 9)
// still fits the ranking kernel's LDS.
constexpr int SPL = 64;
constexpr uint32_t GROUP_SYMS = 50;
constexpr uint32_t MAX_SELECTORS = 32768;

// ---------------------------------------------------------------- phase A
// The scratch rows of the block decode, sized for a whole block of dsz bytes (the file's largest level) whatever a candidate turns
// out to hold: nr rows (<= grid.y, <= what `budget` bytes hold, >= 1) of per_row bytes for nrows block candidates.  mt_tile: ops
// of a move-to-front tile; tab_bytes: a row's table record.
struct RowLayout {
  uint32_t ops_stride, tiles_per_row;
  uint32_t sym_stride;      // symbols in front of the end of block: each emits a byte (but for forgotten runs), so <= dsz
  uint32_t group_tiles, sym_groups;
  uint64_t per_row;
  uint32_t nr;
  bool single;              // one batch holds every row: the decoded rows stay where they are
};
inline RowLayout row_layout(uint32_t dsz, uint32_t nrows, uint64_t budget, uint32_t mt_tile, size_t tab_bytes) {
  RowLayout L;
  L.ops_stride = (dsz + 256u + 255u) & ~255u; L.tiles_per_row = L.ops_stride / mt_tile;
  L.sym_stride = dsz + 4096u;
  L.group_tiles = (std::min<uint32_t>(MAX_SELECTORS, L.sym_stride / GROUP_SYMS + 1u) + 255u) / 256u;
  L.sym_groups = (L.sym_stride + GROUP_SYMS - 1) / GROUP_SYMS;
  L.per_row = (uint64_t)dsz + 6ull * L.ops_stride + 256 + 4 + tab_bytes + MAX_SELECTORS + 4ull * (MAX_SELECTORS + 1) + 2ull * L.sym_groups * GROUP_SYMS;
  L.nr = std::max<uint32_t>(1u, (uint32_t)std::min<uint64_t>(std::min<uint64_t>(nrows ? nrows : 1u, 65535u), std::max<uint64_t>(1ull, budget / L.per_row)));
  L.single = nrows <= L.nr;
  return L;
}

// The row batch that starts at candidate c0: candidates [c0, c1) with at most nr block candidates (kind 0), which hold rows
// r0 .. r0 + rows of the share's numbering (their pad); the end-of-stream candidates behind the last block go with it.
struct RowBatch { uint32_t c0, c1, rows, r0; };
template <typename C>
inline RowBatch row_batch(const C* cands, uint32_t ncand, uint32_t c0, uint32_t nr) {
  RowBatch b{c0, c0, 0, 0};
  while (b.c1 < ncand && (cands[b.c1].kind != 0 || b.rows < nr)) { if (cands[b.c1].kind == 0) { if (!b.rows) b.r0 = cands[b.c1].pad; b.rows++; } b.c1++; }
  return b;
}

// A streaming step's row limit: the candidates in front of bit row_from go, and so does everything from the first block
// candidate past row_limit blocks on.  Returns that candidate's bit (none: ~0).  row_limit ~0: no limit, nothing goes.
template <typename C>
inline uint64_t row_limit_trim(std::vector<C>& cands, uint64_t row_from, uint32_t row_limit) {
  uint64_t cut_bit = ~0ull;
  if (row_limit == ~0u) return cut_bit;
  size_t a = 0, b;
  while (a < cands.size() && cands[a].bit < row_from) a++;
  uint32_t blocks = 0;
  for (b = a; b < cands.size(); b++) if (cands[b].kind == 0 && ++blocks > row_limit) { cut_bit = cands[b].bit; break; }
  cands.erase(cands.begin() + (long)b, cands.end());
  cands.erase(cands.begin(), cands.begin() + (long)a);
  return cut_bit;
}

// ---------------------------------------------------------------- phases B and C
// The inverse-BWT batch [b0, return) of blocks [b0, c1): <= max_el elements (a first block of any size) and <= max_blocks blocks.
// count(k): elements of block k.
template <typename Count>
inline size_t ib_batch_end(size_t b0, size_t c1, uint64_t max_el, size_t max_blocks, Count count) {
  uint64_t el = 0; size_t b = b0;
  while (b < c1 && b - b0 < max_blocks && (b == b0 || el + count(b) <= max_el)) { el += count(b); b++; }
  return b;
}

// The slots of one inverse-BWT batch of nb blocks, count(k) elements in block k.  Blocks of (nearly) one size -- a stream's are,
// but for its last -- get a slot range of that size each (seg_stride) and ONE pass of the sort, segment by segment (strided);
// otherwise they lie back to back and the block number is sorted on too (one or two more passes over everything).  off: a block's
// first slot in the sort / LF arrays; woff: its first byte in the walk's output; M: slots in all; T: radix tiles (tps per
// segment).  rs_tile: slots of a radix tile.
struct IbPlan {
  uint32_t nb = 0, maxc = 0, seg_stride = 0, M = 0, tps = 0;
  uint32_t spl_stride = 0;      // (of this batch: a file of very many small blocks must not pay for the largest level's)
  uint64_t M64 = 0;             // elements of the batch
  size_t T = 0;
  bool strided = false;
  std::vector<uint32_t> off, woff;
  bool fits() const { return M64 < 0xFFFFF000ull; }      // (no: the plan may not run; cannot happen inside the batch limits)
};
template <typename Count>
inline IbPlan ib_plan(uint32_t nb, uint32_t rs_tile, Count count) {
  IbPlan P;
  P.nb = nb; P.off.resize(nb); P.woff.resize(nb);
  for (uint32_t k = 0; k < nb; k++) { P.woff[k] = (uint32_t)P.M64; P.M64 += count(k); P.maxc = std::max<uint32_t>(P.maxc, count(k)); }
  P.seg_stride = (P.maxc + 3u) & ~3u;
  P.spl_stride = P.maxc / SPL + 4;
  P.strided = (uint64_t)nb * P.seg_stride <= P.M64 + P.M64 / 4 && (uint64_t)nb * P.seg_stride < 0xFFFFF000ull;
  P.M = P.strided ? nb * P.seg_stride : (uint32_t)P.M64;
  for (uint32_t k = 0; k < nb; k++) P.off[k] = P.strided ? k * P.seg_stride : P.woff[k];
  P.tps = (P.seg_stride + rs_tile - 1) / rs_tile;
  P.T = P.strided ? (size_t)nb * P.tps + 1 : ((size_t)P.M + rs_tile - 1) / rs_tile + 1;
  return P;
}

}  // namespace cjs
