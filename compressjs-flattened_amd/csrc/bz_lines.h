// bz_lines.h -- the line table of an indexed .bz2 stream behind the C ABI's opaque cjs_bz_lines (lines.hip: create / save / load /
// info, the build and the two questions that run over it).  No HIP in here: line_join.h reads the table on the host.
#pragma once
#include "bz_index.h"
#include <vector>

struct cjs_bz_lines {
  std::vector<uint32_t> nl;       // newlines of block k
  std::vector<uint64_t> cum;      // newlines in front of block k (nl.size() + 1 values: the last is their total)
  uint64_t total_bytes = 0;       // of the index it belongs to ...
  uint32_t crc_fold = 0;          // ... and the fold of that index's stored block CRCs
};

namespace cjs {

constexpr size_t BZ_LINES_HEADER = 40;
// the index entries' stored CRCs folded from 0 as the stream CRC folds them
inline uint32_t bz_lines_fold(const cjs_bz_index* ix) {
  uint32_t c = 0;
  for (const cjs_bz_index_entry& e : ix->e) c = ((c << 1) | (c >> 31)) ^ e.crc;
  return c;
}
// the table of `count` counts for index ix (CJS_E_INVALID_ARG and a detail text if they cannot be that index's)
int bz_lines_make(const cjs_bz_index* ix, const uint32_t* counts, size_t count, cjs_bz_lines** lines);
// whether t is the table of index ix (a detail text if it is not): what every entry point that takes both asks first
bool lines_belong(const cjs_bz_index* ix, const cjs_bz_lines* t);

}  // namespace cjs
