// linekeys.h -- what the line keys (linekeys.hip) offer the two stream consumers built on them, cjs_bzip2_tally
// (tally_stream.hip; §6p) and cjs_bzip2_sort (sort_stream.hip; §6q); LK_PIECE and text_keys_work_bytes come with line_join.h.
#pragma once
#include "range_engine.h"
#include "line_join.h"

namespace cjs {

// The consumer of range_engine that keys the window [first, end) of lines over its touched blocks: the caller names J's destination
// (keys or d_keys, cap), runs the engine with batch() and then J.finish().  h2d / d2h / tiles: what the batches add to the engine's.
struct LineKeysCall {
  const cjs_bz_index* ix; const cjs_bz_lines* t;
  LkJoin J;
  uint64_t h2d = 0, d2h = 0, tiles = 0;
  LineKeysCall(const cjs_bz_index* ix_, const cjs_bz_lines* t_, uint64_t seed, uint64_t first, uint64_t end, const std::vector<uint32_t>& touched) : ix(ix_), t(t_) {
    J.t = t; J.B = lk_bases(seed); J.first = first; J.end = end; J.touched = &touched;
  }
  int batch(const RangeBatch& B);
};

// d_text[0 .. n) -> d_keys (room for key_cap records), in the workspace d_work of text_keys_work_bytes(n, piece) bytes, on stream s.
// tally_tail: the tally's rule for the tail (an empty one is no line, another is keyed with a newline), else a record for the tail
// whatever it is, as cjs_stage_line_keys gives one.  *n_keys = the records written.  Returns with s drained.
int text_keys_device(hipStream_t s, const uint8_t* d_text, size_t n, const LkBases& B, size_t piece, bool tally_tail, cjs_bz_linekey* d_keys, size_t key_cap,
                     uint8_t* d_work, uint64_t* n_keys, uint64_t* h2d, uint64_t* d2h);

// The fills and the patches of a finished join onto its device array J.d_keys, queued on stream s (nothing is waited for: J lives
// until s is drained).  d_patch: device room for max_patches patches.
int lk_apply_join(hipStream_t s, const LkJoin& J, LkPatch* d_patch, size_t max_patches);

// The window's cut as text in device memory: cjs_bzip2_cut_device into a pooled buffer of the touched blocks' bytes + 1 (never less
// than the window's bytes + 1, which the cut's contract says is enough).  touched: line_window_blocks of the window, which are the
// blocks the cut itself decodes.  The host form's stream goes up first, as the passes would take it.
inline size_t cut_text_bound(const cjs_bz_index* idx, const std::vector<uint32_t>& touched) { size_t b = 1; for (uint32_t k : touched) b += idx->e[k].size; return b; }
struct CutText {
  DevBuf d_stream, d_text;
  size_t bound, n = 0;                                      // the room of d_text; the bytes the cut wrote
  CutText(bool host, size_t stream_bytes, size_t bound_) : d_stream(host ? std::max<size_t>(stream_bytes, 1) : 1), d_text(bound_), bound(bound_) {}
  // in (h2d += its bytes) or d_in, on device dev.  Returns the cut's code, with the cut's detail; info gets the cut's verdict on the blocks.
  template <typename Info>
  int run(const uint8_t* in, const uint8_t* d_in, size_t n_in, const cjs_bz_index* idx, const cjs_bz_lines* t, uint64_t first, uint64_t count, uint32_t mode,
          uint32_t delim, const cjs_cut_range* sel, uint32_t nsel, int dev, uint64_t& h2d, Info* info) {
    if (in && hipMemcpy(d_stream.p, in, n_in, hipMemcpyHostToDevice) != hipSuccess) return CJS_E_HIP;
    h2d += in ? n_in : 0;
    cjs_opts here{};                                        // the cut runs on the device this call has selected
    here.struct_size = sizeof here; here.device = dev;
    cjs_bz_cut_info ci;
    const int rc = cjs_bzip2_cut_device(in ? (const uint8_t*)d_stream.p : d_in, n_in, idx, t, first, count, mode, delim, sel, nsel, (uint8_t*)d_text.p, bound, &n, &ci, &here);
    info->blocks_decoded = ci.blocks_decoded; info->n_bad_blocks = ci.n_bad_blocks; info->first_bad_block = ci.first_bad_block;
    return rc;
  }
};

}  // namespace cjs
