// bz_index.h -- the block index of a .bz2 stream behind the C ABI's opaque cjs_bz_index (bz_index.hip: create / save / load / info;
// range.hip: cjs_bzip2_index_build and the range reads that run over it).
#pragma once
#include "cjs_hip.h"
#include <vector>

struct cjs_bz_index {
  std::vector<cjs_bz_index_entry> e;      // one per block, stream order
  std::vector<uint64_t> off;              // decoded offset of block k (e.size() + 1 values: the last is total_bytes)
  uint64_t stream_bytes = 0;
  bool multistream = false;
};

namespace cjs {

constexpr size_t BZ_INDEX_HEADER = 32;
// the index of `count` validated entries (CJS_E_INVALID_ARG and a detail text for the first rule one of them breaks)
int bz_index_make(const cjs_bz_index_entry* entries, size_t count, uint64_t stream_bytes, bool multistream, cjs_bz_index** idx);

}  // namespace cjs
