// sort.h -- what the line sort (sort.hip) offers the stream consumer that feeds it a cut in device memory
// (cjs_bzip2_sort, sort_stream.hip): its two workspaces, sized from the text's bytes and from the number of lines, and the two steps.
#pragma once
#include <functional>
#include "cjs_internal.h"
#include "sort_plan.h"

namespace cjs {

enum SlScalar { SL_NL = 0, SL_TAIL = 1, SL_NACT = 2, SL_NGRP = 3, SL_ND = 4, SL_UBYTES = 5, SL_TEXT = 6, SL_SPARE = 7, SL_SCALARS = 8 };

// the counting step's workspace: a count per 4 KiB tile of the text
struct SortCount {
  uint64_t *tc = nullptr, *scal = nullptr;
  static size_t bytes_needed(size_t text_bytes) { return sl_count_bytes(text_bytes); }
  int carve(Arena& a, size_t text_bytes) {
    tc = a.take<uint64_t>(sl_text_tiles(text_bytes) + 1); scal = a.take<uint64_t>(SL_SCALARS);
    return tc && scal ? 0 : (int)CJS_E_OUT_OF_MEMORY;
  }
};
// the rounds' workspace for up to `lines` lines: sl_lines_bytes and the sorter's histograms
struct SortWork {
  uint64_t *tcnt = nullptr, *taux = nullptr, *scal = nullptr;
  uint32_t *start = nullptr, *order = nullptr;
  uint8_t *head = nullptr, *aflag = nullptr;
  uint64_t *key[2] = {nullptr, nullptr}, *wsave = nullptr;
  uint32_t *val[2] = {nullptr, nullptr}, *gk[2] = {nullptr, nullptr};
  uint32_t* dense[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};      // [which][slot, line, group]
  uint32_t *gpos = nullptr, *eline = nullptr;
  uint64_t* off = nullptr;
  size_t lines = 0;
  RadixWork rs;
  static size_t bytes_needed(size_t lines) {
    const size_t L = lines ? lines : 1;
    return sl_lines_bytes(L) + sl_pad(4 * RadixWork::hist_words(RadixWork::hist_tiles_for(L))) + sl_pad(4 * 256);
  }
  int carve(Arena& a, size_t n_lines) {
    const size_t L = n_lines ? n_lines : 1;
    lines = L;
    tcnt = a.take<uint64_t>(sl_tiles(L) + 1); taux = a.take<uint64_t>(sl_tiles(L) + 1); scal = a.take<uint64_t>(SL_SCALARS);
    start = a.take<uint32_t>(L + 1); order = a.take<uint32_t>(L);
    head = a.take<uint8_t>(L); aflag = a.take<uint8_t>(L);
    bool ok = tcnt && taux && scal && start && order && head && aflag;
    for (int i = 0; i < 2; i++) {
      key[i] = a.take<uint64_t>(L); val[i] = a.take<uint32_t>(L); gk[i] = a.take<uint32_t>(L);
      ok = ok && key[i] && val[i] && gk[i];
      for (int k = 0; k < 3; k++) ok = (dense[i][k] = a.take<uint32_t>(L)) && ok;
    }
    wsave = a.take<uint64_t>(L); gpos = a.take<uint32_t>(L); eline = a.take<uint32_t>(L); off = a.take<uint64_t>(L + 1);
    if (!ok || !wsave || !gpos || !eline || !off) return CJS_E_OUT_OF_MEMORY;
    return rs.carve(a, RadixWork::hist_tiles_for(L), 1);
  }
};

struct SortStats { uint64_t h2d = 0, d2h = 0; };
// What a sort is asked for.  d_lines / d_counts: device arrays with room for min(cap, the lines) entries (d_counts may be null).
// text(need, &d_out): called once when text is wanted and its size is known; it names need bytes of device memory or fails the
// call (CJS_E_OUTPUT_TOO_SMALL).  An empty function: no text.
struct SortCall {
  const uint8_t* d_text = nullptr; size_t n = 0;
  uint32_t flags = 0; uint64_t base = 0;
  uint64_t *d_lines = nullptr, *d_counts = nullptr; size_t cap = 0;
  std::function<int(uint64_t, uint8_t**)> text;
};

// d_text[0 .. n), 0 < n <= SL_MAX_BYTES: *lines = its lines by the tail rule.  Leaves the scanned tile counts in c.  Returns with s drained.
int sort_count(hipStream_t s, SortCount& c, const uint8_t* d_text, size_t n, uint64_t* lines, SortStats& st);
// ... then the sort of those lines (0 < lines <= w.lines), the emit and the gather: info's n_lines, n_out, n_distinct, text_bytes,
// rounds; *text_n = the bytes of text written (or needed).  Returns with s drained.
int sort_run(hipStream_t s, SortWork& w, const SortCount& c, const SortCall& q, uint64_t lines, uint64_t* text_n, cjs_bz_sort_info* info, SortStats& st);

}  // namespace cjs
