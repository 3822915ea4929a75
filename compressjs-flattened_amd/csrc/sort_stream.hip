// sort_stream.hip -- the lines of an indexed .bz2 stream ordered by content (cjs_bzip2_sort[_device]): the window's cut
// as text in device memory (linekeys.h: CutText), sorted there (sort.h).  No kernel of its own.
#include "linekeys.h"
#include "sort.h"
#include "cut_plan.h"
#include <algorithm>

using namespace cjs;

namespace {

// A composition in the manner of the tally of a cut: the cut as device text (whole lines: the cut with bytes 1-), then the line
// sort of that text (sort.hip), line numbers raised by the window's first.  Everything is sized from the tables and taken before
// the cut runs.  lines_out / counts_out are host memory; the text goes to *text_out (host form: allocated here) or to d_text_out.
int sort_core(const uint8_t* in, const uint8_t* d_in, size_t n, const cjs_bz_index* idx, const cjs_bz_lines* t, uint64_t first, uint64_t count, uint32_t mode,
              uint32_t delim, const cjs_cut_range* sel, uint32_t nsel, uint32_t flags, uint64_t* lines_out, uint64_t* counts_out, size_t cap, uint8_t** text_out,
              uint8_t* d_text_out, size_t text_cap, size_t* text_n, cjs_bz_sort_info* info, const cjs_opts* opts, uint64_t max_bytes, uint64_t max_lines) {
  clear_detail();
  if (!idx || !t || !info || (!lines_out && cap) || !sl_flags_ok(flags)) return CJS_E_INVALID_ARG;
  const cjs_cut_range whole{1u, 0xFFFFFFFFu};
  if (mode == CJS_SORT_LINES) { mode = CJS_CUT_BYTES; delim = 0; sel = &whole; nsel = 1; }
  { CtSel S; CJS_TRY(ct_normalise(mode, delim, sel, nsel, &S)); }      // (the cut's checks; an unknown mode is refused there)
  CJS_TRY(check_index_stream(in ? in : d_in, n, idx));
  if (!lines_belong(idx, t)) return CJS_E_INVALID_ARG;
  sl_info_clear(info);
  const bool want_text = text_n != nullptr;
  if (want_text) *text_n = 0;
  HostBuf host;
  const uint64_t end = line_window_end(first, count, t->cum.back());
  const std::vector<uint32_t> touched = line_window_blocks(t->cum, t->total_bytes, idx->off, first, end);
  info->blocks_decoded = touched.size();
  if (touched.empty()) {      // an empty window, or a stream without a block: its one line is the empty tail, which is no line
    if (text_out && !(*text_out = HostBuf(1).release())) return CJS_E_OUT_OF_MEMORY;
    return 0;
  }
  const uint64_t nwin = end - first;
  const size_t bound = cut_text_bound(idx, touched), room = (size_t)std::min<uint64_t>(cap, nwin);
  if (bound - 1 > std::min<uint64_t>(max_bytes, SL_MAX_BYTES) || nwin > std::min<uint64_t>(max_lines, SL_MAX_LINES)) return CJS_E_UNSUPPORTED;
  CallDevice cd;
  CJS_TRY(cd.select(opts));
  if (d_in && !on_device(d_in, cd.dev)) return CJS_E_INVALID_ARG;      // (no host pointer reaches a kernel)
  if (d_text_out && !on_device(d_text_out, cd.dev)) return CJS_E_INVALID_ARG;
  CutText cut(in != nullptr, n, bound);
  DevBuf d_lines(8 * std::max<size_t>(room, 1)), d_counts(counts_out ? 8 * std::max<size_t>(room, 1) : 8), d_out(text_out ? bound : 1);
  Arena ca, wa; SortCount c; SortWork w;
  if (!cut.d_stream.p || !cut.d_text.p || !d_lines.p || !d_counts.p || !d_out.p) return CJS_E_OUT_OF_MEMORY;
  CJS_TRY(ca.init_pooled(SortCount::bytes_needed(bound)));
  CJS_TRY(c.carve(ca, bound));
  CJS_TRY(wa.init_pooled(SortWork::bytes_needed((size_t)nwin)));
  CJS_TRY(w.carve(wa, (size_t)nwin));
  SortStats cut_st, st;
  CJS_TRY(cut.run(in, d_in, n, idx, t, first, count, mode, delim, sel, nsel, cd.dev, cut_st.h2d, info));
  Stream s;
  CJS_HIP_TRY(hipStreamCreate(s.put()));
  uint64_t L = 0;
  if (cut.n) CJS_TRY(sort_count(s, c, (const uint8_t*)cut.d_text.p, cut.n, &L, st));
  if (L > nwin) return CJS_E_HIP;                           // (cannot be: the cut writes a line per line of the window at most)
  int rc = 0; size_t tn = 0;
  if (L) {
    SortCall q;
    q.d_text = (const uint8_t*)cut.d_text.p; q.n = cut.n; q.flags = flags; q.base = first; q.d_lines = (uint64_t*)d_lines.p;
    q.d_counts = counts_out ? (uint64_t*)d_counts.p : nullptr; q.cap = cap;
    if (want_text)
      q.text = [&](uint64_t need, uint8_t** p) {
        *p = text_out ? (uint8_t*)d_out.p : d_text_out;
        return !text_out && need > text_cap ? (int)CJS_E_OUTPUT_TOO_SMALL : 0;
      };
    rc = sort_run(s, w, c, q, L, &tn, info, st);
    if (want_text) *text_n = tn;
    if (rc && rc != CJS_E_OUTPUT_TOO_SMALL) return rc;
    const size_t m = (size_t)std::min<uint64_t>(cap, info->n_out);
    int rc2 = 0;
    if (!rc && text_out && !(host = HostBuf(std::max<size_t>(tn, 1)))) rc2 = CJS_E_OUT_OF_MEMORY;
    if (!rc2 && m && (hipMemcpyAsync(lines_out, d_lines.p, 8 * m, hipMemcpyDeviceToHost, s) != hipSuccess ||
                      (counts_out && hipMemcpyAsync(counts_out, d_counts.p, 8 * m, hipMemcpyDeviceToHost, s) != hipSuccess))) rc2 = CJS_E_HIP;
    if (!rc && !rc2 && text_out && tn && hipMemcpyAsync(host.p, d_out.p, tn, hipMemcpyDeviceToHost, s) != hipSuccess) rc2 = CJS_E_HIP;
    CJS_TRY(drained(s, rc2));
    st.d2h += 8 * m * (counts_out ? 2 : 1) + (text_out ? tn : 0);
  } else if (text_out && !(host = HostBuf(1))) return CJS_E_OUT_OF_MEMORY;
  if (text_out && !rc) *text_out = host.release();
  if (env_debug())
    fprintf(stderr, "[cjs sort] %s: lines [%llu, %llu), %zu of %zu blocks touched, %zu text bytes, %llu lines, %llu distinct, %llu out, %llu rounds, upload %llu, "
            "beyond the cut: H2D %llu D2H %llu\n", d_in ? "device" : "host", (unsigned long long)first, (unsigned long long)end, touched.size(), idx->e.size(), cut.n,
            (unsigned long long)info->n_lines, (unsigned long long)info->n_distinct, (unsigned long long)info->n_out, (unsigned long long)info->rounds,
            (unsigned long long)cut_st.h2d, (unsigned long long)st.h2d, (unsigned long long)st.d2h);
  return rc;
}

}  // namespace

extern "C" int cjs_bzip2_sort(const uint8_t* in, size_t n, const cjs_bz_index* idx, const cjs_bz_lines* lines, uint64_t first, uint64_t count, uint32_t mode,
                              uint32_t delim, const cjs_cut_range* sel, uint32_t nsel, uint32_t flags, uint64_t* lines_out, uint64_t* counts_out, size_t cap,
                              uint8_t** text_out, size_t* text_n, cjs_bz_sort_info* info, const cjs_opts* opts) {
  CJS_GUARD_BEGIN
  if ((!in && n) || (text_out != nullptr) != (text_n != nullptr)) return CJS_E_INVALID_ARG;
  if (text_out) *text_out = nullptr;
  return sort_core(in ? in : (const uint8_t*)"", nullptr, n, idx, lines, first, count, mode, delim, sel, nsel, flags, lines_out, counts_out, cap, text_out, nullptr, 0,
                   text_n, info, opts, SL_MAX_BYTES, SL_MAX_LINES);
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

extern "C" int cjs_bzip2_sort_device(const uint8_t* d_in, size_t n, const cjs_bz_index* idx, const cjs_bz_lines* lines, uint64_t first, uint64_t count, uint32_t mode,
                                     uint32_t delim, const cjs_cut_range* sel, uint32_t nsel, uint32_t flags, uint64_t* lines_out, uint64_t* counts_out, size_t cap,
                                     uint8_t* d_text_out, size_t text_cap, size_t* text_n, cjs_bz_sort_info* info, const cjs_opts* opts) {
  CJS_GUARD_BEGIN
  if ((!d_in && n) || (!d_text_out && text_cap) || (d_text_out && !text_n)) return CJS_E_INVALID_ARG;
  return sort_core(nullptr, d_in, n, idx, lines, first, count, mode, delim, sel, nsel, flags, lines_out, counts_out, cap, nullptr, d_text_out, text_cap, text_n, info,
                   opts, SL_MAX_BYTES, SL_MAX_LINES);
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

// EXISTS FOR TESTS: the whole-line stream sort with the limits on the touched blocks' bytes and the window's lines as arguments
// (no fixture of 2^32 bytes fits a test).  Exactly one of in / d_in.
extern "C" int cjs_stage_bzip2_sort_limit(const uint8_t* in, const uint8_t* d_in, size_t n, const cjs_bz_index* idx, const cjs_bz_lines* lines, uint64_t first,
                                          uint64_t count, uint64_t max_bytes, uint64_t max_lines, uint32_t flags, uint64_t* lines_out, uint64_t* counts_out, size_t cap,
                                          cjs_bz_sort_info* info, const cjs_opts* opts) {
  CJS_GUARD_BEGIN
  if ((in != nullptr) == (d_in != nullptr)) return CJS_E_INVALID_ARG;
  return sort_core(in, d_in, n, idx, lines, first, count, CJS_SORT_LINES, 0, nullptr, 0, flags, lines_out, counts_out, cap, nullptr, nullptr, 0, nullptr, info, opts,
                   max_bytes, max_lines);
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}
