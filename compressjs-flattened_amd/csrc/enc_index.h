// enc_index.h -- the block rows of the compress pipeline (enc_index.hip): what the indexed compress entry points ask
// of a context besides the stream, and how the rows become a cjs_bz_index and a cjs_bz_lines.  The arithmetic is enc_index_plan.h.
#pragma once
#include "cjs_internal.h"
#include "enc_index_plan.h"
#include <vector>

struct cjs_ctx;
struct cjs_bz_index;
struct cjs_bz_lines;

namespace cjs {

// The row storage of a context: room for range_blocks rows on the device and their pinned twin.  Made by the first indexed call on
// the context (enc_rows_enqueue); a context that is never asked has none.
struct EncRowsWork {
  DevMem<EncRow> d;
  Pinned<EncRow> h;
  size_t cap = 0;
};
void enc_rows_destroy(EncRowsWork* w);
struct EncRowsDelete { void operator()(EncRowsWork* w) const { enc_rows_destroy(w); } };

// What an indexed call hands down to the pipeline and gets back: the rows of the blocks the call packed, in stream order.
struct EncRowsWant {
  bool lines = false;                 // count the newlines too (one more read of the input)
  std::vector<EncRow> rows;
};

// Behind blocks_through_tables (and the join of the block CRCs) on the context's stream: the rows of blocks [f, f + cnt) of the
// stream whose boundaries c->rle holds, made on the device and copied to the context's pinned rows.  Nothing here waits; once
// the stream has drained, enc_rows_collect appends them to want.rows.
int enc_rows_enqueue(cjs_ctx* c, const uint8_t* d_in, size_t n, uint32_t f, uint32_t cnt, bool lines);
void enc_rows_collect(const cjs_ctx* c, uint32_t cnt, EncRowsWant& want);

// The tables of a finished stream: entries / newlines (enc_rows_append) whose last block ends at end_bit.  lines may be null.
// The entries go through bz_index_make and bz_lines_make, which check every one: a refusal there is a fault of the library,
// CJS_E_HIP.  On failure *idx and *lines are null.
int enc_tables_make(const std::vector<cjs_bz_index_entry>& entries, const std::vector<uint32_t>& newlines, uint64_t end_bit,
                    cjs_bz_index** idx, cjs_bz_lines** lines);

}  // namespace cjs
