// bz_index.hip -- cjs_bz_index: the host half of the indexed range reads (include/cjs_hip.h).  No device is touched here:
// an index is made from a caller's entries or from its serialised form, checked entry by entry, and handed out again.
// cjs_bzip2_index_build (one table pass on the GPU) and the range reads are in range.hip.
#include "cjs_internal.h"
#include "bz_index.h"
#include <algorithm>
#include <stdlib.h>
#include <string.h>

using namespace cjs;

static_assert(sizeof(cjs_bz_index_entry) == 32, "the entry is the serialised entry");

namespace {

const char IX_MAGIC[8] = {'C', 'J', 'S', 'B', 'Z', 'I', 'X', '1'};
constexpr uint32_t IX_VERSION = 1, IX_FLAG_MULTISTREAM = 1;

void put_le(uint8_t* p, uint64_t v, int bytes) { for (int i = 0; i < bytes; i++) p[i] = (uint8_t)(v >> (8 * i)); }
uint64_t get_le(const uint8_t* p, int bytes) { uint64_t v = 0; for (int i = 0; i < bytes; i++) v |= (uint64_t)p[i] << (8 * i); return v; }

}  // namespace

namespace cjs {

int bz_index_make(const cjs_bz_index_entry* entries, size_t count, uint64_t stream_bytes, bool multistream, cjs_bz_index** idx) {
  *idx = nullptr;
  if (stream_bytes > (~0ull >> 3)) { set_detail("stream size out of range"); return CJS_E_INVALID_ARG; }
  uint64_t last_end = 0;
  for (size_t k = 0; k < count; k++) {
    const cjs_bz_index_entry& e = entries[k];
    const char* why = nullptr;
    if (e.bitpos < 32) why = "block starts inside the stream header";
    else if (e.bitpos < last_end) why = "blocks not ascending";
    else if (e.end_bit <= e.bitpos + 48 + 32) why = "block too short";
    else if (e.end_bit > 8 * stream_bytes) why = "block ends behind the stream";
    else if (e.level < 1 || e.level > 9) why = "level out of range";
    else if (e.size > 52u * 100000u * e.level) why = "size too large for the level";
    else if (e.reserved != 0) why = "reserved field not zero";
    if (why) { set_detail("index entry %zu: %s", k, why); return CJS_E_INVALID_ARG; }
    last_end = e.end_bit;
  }
  cjs_bz_index* ix = new cjs_bz_index;
  ix->e.assign(entries, entries + count);
  ix->off.assign(count + 1, 0);
  for (size_t k = 0; k < count; k++) ix->off[k + 1] = ix->off[k] + entries[k].size;
  ix->stream_bytes = stream_bytes; ix->multistream = multistream;
  *idx = ix;
  return 0;
}

}  // namespace cjs

extern "C" int cjs_bzip2_index_create(const cjs_bz_index_entry* entries, size_t count, uint64_t stream_bytes, int multistream, cjs_bz_index** idx) {
  if (!idx || (!entries && count)) return CJS_E_INVALID_ARG;
  clear_detail();
  CJS_GUARD_BEGIN
  return bz_index_make(entries, count, stream_bytes, multistream != 0, idx);
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_INVALID_ARG)
}

extern "C" int cjs_bzip2_index_save(const cjs_bz_index* idx, uint8_t** bytes, size_t* nbytes) {
  if (!idx || !bytes || !nbytes) return CJS_E_INVALID_ARG;
  const size_t count = idx->e.size(), total = BZ_INDEX_HEADER + 32 * count;
  uint8_t* p = (uint8_t*)malloc(total);
  if (!p) return CJS_E_OUT_OF_MEMORY;
  memcpy(p, IX_MAGIC, 8);
  put_le(p + 8, IX_VERSION, 4);
  put_le(p + 12, idx->multistream ? IX_FLAG_MULTISTREAM : 0u, 4);
  put_le(p + 16, idx->stream_bytes, 8);
  put_le(p + 24, count, 8);
  for (size_t k = 0; k < count; k++) {
    const cjs_bz_index_entry& e = idx->e[k];
    uint8_t* q = p + BZ_INDEX_HEADER + 32 * k;
    put_le(q, e.bitpos, 8); put_le(q + 8, e.end_bit, 8); put_le(q + 16, e.size, 4); put_le(q + 20, e.crc, 4); put_le(q + 24, e.level, 4); put_le(q + 28, e.reserved, 4);
  }
  *bytes = p; *nbytes = total;
  return 0;
}

extern "C" int cjs_bzip2_index_load(const uint8_t* bytes, size_t nbytes, cjs_bz_index** idx) {
  if (!idx || (!bytes && nbytes)) return CJS_E_INVALID_ARG;
  *idx = nullptr;
  clear_detail();
  CJS_GUARD_BEGIN
  if (nbytes < BZ_INDEX_HEADER || memcmp(bytes, IX_MAGIC, 8) != 0) { set_detail("not a block index: bad magic"); return CJS_E_INVALID_ARG; }
  if (get_le(bytes + 8, 4) != IX_VERSION) { set_detail("block index: unknown version"); return CJS_E_INVALID_ARG; }
  const uint32_t flags = (uint32_t)get_le(bytes + 12, 4);
  if (flags & ~IX_FLAG_MULTISTREAM) { set_detail("block index: undefined flag bits"); return CJS_E_INVALID_ARG; }
  const uint64_t stream_bytes = get_le(bytes + 16, 8), count = get_le(bytes + 24, 8);
  if (count != (nbytes - BZ_INDEX_HEADER) / 32 || (nbytes - BZ_INDEX_HEADER) % 32) { set_detail("block index: length does not match the entry count"); return CJS_E_INVALID_ARG; }
  std::vector<cjs_bz_index_entry> e((size_t)count);
  for (size_t k = 0; k < (size_t)count; k++) {
    const uint8_t* q = bytes + BZ_INDEX_HEADER + 32 * k;
    e[k].bitpos = get_le(q, 8); e[k].end_bit = get_le(q + 8, 8); e[k].size = (uint32_t)get_le(q + 16, 4); e[k].crc = (uint32_t)get_le(q + 20, 4);
    e[k].level = (uint32_t)get_le(q + 24, 4); e[k].reserved = (uint32_t)get_le(q + 28, 4);
  }
  return bz_index_make(e.data(), e.size(), stream_bytes, (flags & IX_FLAG_MULTISTREAM) != 0, idx);
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_INVALID_ARG)
}

extern "C" int cjs_bzip2_index_info(const cjs_bz_index* idx, uint64_t* blocks, uint64_t* total_bytes, uint64_t* stream_bytes, int* multistream) {
  if (!idx) return CJS_E_INVALID_ARG;
  if (blocks) *blocks = idx->e.size();
  if (total_bytes) *total_bytes = idx->off.back();
  if (stream_bytes) *stream_bytes = idx->stream_bytes;
  if (multistream) *multistream = idx->multistream ? 1 : 0;
  return 0;
}

extern "C" long cjs_bzip2_index_entries(const cjs_bz_index* idx, cjs_bz_index_entry* entries, long cap) {
  if (!idx || (!entries && cap > 0)) return CJS_E_INVALID_ARG;
  const size_t m = std::min<size_t>(idx->e.size(), cap > 0 ? (size_t)cap : 0);
  if (m) memcpy(entries, idx->e.data(), m * sizeof(cjs_bz_index_entry));
  return (long)idx->e.size();
}

extern "C" void cjs_bzip2_index_destroy(cjs_bz_index* idx) { delete idx; }
