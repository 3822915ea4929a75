// tally_stream.hip -- the frequency table of the lines of an indexed .bz2 stream (cjs_bzip2_tally[_device]): the
// keys of the window's lines (linekeys.h) left in device memory, grouped there (tally.h).  No kernel of its own.
#include "linekeys.h"
#include "tally.h"
#include "cut_plan.h"
#include <algorithm>

using namespace cjs;

namespace {

// The tally of a cut (modes CJS_CUT_FIELDS / CJS_CUT_BYTES), a composition: the cut as device text (CutText), the keys of that
// text's lines (text_keys_device), the grouping.  A bad block fails the call as it fails the cut.  Everything is sized from the
// tables and taken before the cut runs.
int tally_cut(const uint8_t* in, const uint8_t* d_in, size_t n, const cjs_bz_index* idx, const cjs_bz_lines* t, uint64_t first, uint64_t end, uint64_t count,
              uint64_t seed, uint32_t mode, uint32_t delim, const cjs_cut_range* sel, uint32_t nsel, uint32_t order, uint64_t min_count, uint64_t max_count,
              cjs_bz_tally* out, size_t cap, cjs_bz_tally_info* info, const std::vector<uint32_t>& touched, int dev) {
  const uint64_t nwin = end - first;
  CutText cut(in != nullptr, n, cut_text_bound(idx, touched));
  const size_t work = text_keys_work_bytes(cut.bound, LK_PIECE), max_groups = (size_t)std::min<uint64_t>(cap, nwin);
  DevBuf d_keys(sizeof(cjs_bz_linekey) * ((size_t)nwin + 1)), d_work(work), d_stage(sizeof(cjs_bz_tally) * std::max<size_t>(max_groups, 1));
  Arena arena; TallyWork w;
  if (!cut.d_stream.p || !cut.d_text.p || !d_keys.p || !d_work.p || !d_stage.p) return CJS_E_OUT_OF_MEMORY;
  CJS_TRY(arena.init_pooled(TallyWork::bytes_needed((size_t)nwin)));
  CJS_TRY(w.carve(arena, (size_t)nwin));
  uint64_t h2d = 0, d2h = 0;
  CJS_TRY(cut.run(in, d_in, n, idx, t, first, count, mode, delim, sel, nsel, dev, h2d, info));
  Stream s;
  CJS_HIP_TRY(hipStreamCreate(s.put()));
  uint64_t nkeys = 0;
  CJS_TRY(text_keys_device(s, (const uint8_t*)cut.d_text.p, cut.n, lk_bases(seed), LK_PIECE, true, (cjs_bz_linekey*)d_keys.p, (size_t)nwin + 1, (uint8_t*)d_work.p, &nkeys, &h2d, &d2h));
  cjs_tally_info ti{nkeys, 0, 0, 0, 0};
  if (nkeys) CJS_TRY(tally_to_host(s, w, (const cjs_bz_linekey*)d_keys.p, (uint32_t)nkeys, order, min_count, max_count, first, out, cap, &ti, (cjs_bz_tally*)d_stage.p));
  info->n_lines = nkeys; info->n_bad_lines = ti.n_bad; info->n_distinct = ti.n_distinct; info->n_groups = ti.n_groups; info->max_count = ti.max_count;
  if (env_debug())
    fprintf(stderr, "[cjs tally] %s: lines [%llu, %llu), mode %s, %zu of %zu blocks touched, %zu text bytes in %zu pieces, %llu distinct, %llu kept, beyond the cut: "
            "H2D %llu D2H %llu\n", d_in ? "device" : "host", (unsigned long long)first, (unsigned long long)end, mode == CJS_CUT_FIELDS ? "fields" : "bytes", touched.size(),
            idx->e.size(), cut.n, text_keys_pieces(cut.n, LK_PIECE), (unsigned long long)ti.n_distinct, (unsigned long long)ti.n_groups, (unsigned long long)h2d,
            (unsigned long long)(d2h + 8 * TL_SCALARS + sizeof(cjs_bz_tally) * std::min<uint64_t>(cap, ti.n_groups)));
  return 0;
}

// cjs_bzip2_tally[_device]: the passes of the line keys with the records kept in a device array of the window's lines, then the
// fills and patches of the join, then the grouping (tally.hip).  All device memory beyond a pass's is sized from the table and
// taken before the first pass: 16 bytes per line of the window for the records, TallyWork::bytes_needed for the grouping, 24 bytes
// per touched block for the patches and 32 bytes per group that can come down (min(cap, the window's lines)).
// max_lines: the most lines a window may have (TL_MAX_KEYS; the test hook lowers it)
int tally_core(const uint8_t* in, const uint8_t* d_in, size_t n, const cjs_bz_index* idx, const cjs_bz_lines* t, uint64_t first, uint64_t count, uint64_t seed,
               uint32_t mode, uint32_t delim, const cjs_cut_range* sel, uint32_t nsel, uint32_t order, uint64_t min_count, uint64_t max_count, cjs_bz_tally* out,
               size_t cap, cjs_bz_tally_info* info, const cjs_opts* opts, uint64_t max_lines) {
  clear_detail();
  if (!idx || !t || !info || (!out && cap) || !tl_args_ok(order, min_count, max_count)) return CJS_E_INVALID_ARG;
  if (mode != CJS_TALLY_LINES) { CtSel S; CJS_TRY(ct_normalise(mode, delim, sel, nsel, &S)); }      // (the cut's checks; an unknown mode is refused there)
  CJS_TRY(check_index_stream(in ? in : d_in, n, idx));
  if (!lines_belong(idx, t)) return CJS_E_INVALID_ARG;
  *info = cjs_bz_tally_info{0, 0, 0, 0, 0, 0, 0, ~0ull};
  const uint64_t end = line_window_end(first, count, t->cum.back());
  if (first >= end) return 0;
  const uint64_t nwin = end - first;
  if (nwin > std::min<uint64_t>(max_lines, TL_MAX_KEYS)) return CJS_E_UNSUPPORTED;
  const std::vector<uint32_t> touched = line_window_blocks(t->cum, t->total_bytes, idx->off, first, end);
  info->blocks_decoded = touched.size();
  if (touched.empty()) return 0;      // a stream without a block: its one line is the empty tail, which is no line
  CallDevice cd;
  CJS_TRY(cd.select(opts));
  if (d_in && !on_device(d_in, cd.dev)) return CJS_E_INVALID_ARG;      // (no host pointer reaches a kernel)
  if (mode != CJS_TALLY_LINES)
    return tally_cut(in, d_in, n, idx, t, first, end, count, seed, mode, delim, sel, nsel, order, min_count, max_count, out, cap, info, touched, cd.dev);
  DevBuf d_keys(sizeof(cjs_bz_linekey) * (size_t)nwin);
  Arena arena; TallyWork w;
  if (!d_keys.p) return CJS_E_OUT_OF_MEMORY;
  CJS_TRY(arena.init_pooled(TallyWork::bytes_needed((size_t)nwin)));
  CJS_TRY(w.carve(arena, (size_t)nwin));
  // ... and the patches (at most one per touched block, and the tail) and the groups on their way down
  const size_t max_patches = touched.size() + 1, max_groups = (size_t)std::min<uint64_t>(cap, nwin);
  DevBuf d_patch(sizeof(LkPatch) * max_patches), d_stage(sizeof(cjs_bz_tally) * std::max<size_t>(max_groups, 1));
  if (!d_patch.p || !d_stage.p) return CJS_E_OUT_OF_MEMORY;
  LineKeysCall C(idx, t, seed, first, end, touched);
  C.J.cap = (size_t)nwin; C.J.d_keys = (cjs_bz_linekey*)d_keys.p;
  RangeStats st; RangeVerdicts V(idx);
  CJS_TRY(range_engine(in, d_in, idx, touched, V, cd.dev, st, [&](const RangeBatch& B) { return C.batch(B); }));
  C.J.finish();
  const BadBlocks bad = V.bad_among(touched);
  info->n_bad_blocks = bad.n; info->first_bad_block = bad.first;
  // every pass has drained its stream: the fills, the patches and the grouping go on one of their own
  Stream s;
  CJS_HIP_TRY(hipStreamCreate(s.put()));
  int rc = lk_apply_join(s, C.J, (LkPatch*)d_patch.p, max_patches);
  const size_t np = C.J.patches.size();
  const uint64_t nkeys = nwin - (C.J.tail_dropped ? 1 : 0);
  cjs_tally_info ti{nkeys, 0, 0, 0, 0};
  if (!rc && nkeys) rc = tally_to_host(s, w, C.J.d_keys, (uint32_t)nkeys, order, min_count, max_count, first, out, cap, &ti, (cjs_bz_tally*)d_stage.p);
  else rc = drained(s, rc);
  CJS_TRY(rc);
  info->n_lines = nkeys; info->n_bad_lines = ti.n_bad; info->n_distinct = ti.n_distinct; info->n_groups = ti.n_groups; info->max_count = ti.max_count;
  if (bad.n) V.set_bad_detail(idx, (size_t)bad.first);
  if (env_debug())
    fprintf(stderr, "[cjs tally] %s: lines [%llu, %llu), mode lines, %zu of %zu blocks touched, %llu bad, %u passes (%u row batches, %u inverse-BWT batches), upload %llu B, "
            "%llu tiles, %llu bad lines, %llu distinct, %llu kept, %zu patches, %zu fills, H2D %llu D2H %llu\n", d_in ? "device" : "host", (unsigned long long)first,
            (unsigned long long)end, touched.size(), idx->e.size(), (unsigned long long)bad.n, st.passes, st.a_batches, st.b_batches, (unsigned long long)st.up,
            (unsigned long long)C.tiles, (unsigned long long)ti.n_bad, (unsigned long long)ti.n_distinct, (unsigned long long)ti.n_groups, np, C.J.fills.size(),
            (unsigned long long)(st.h2d + C.h2d + sizeof(LkPatch) * np),
            (unsigned long long)(st.d2h + C.d2h + 8 * TL_SCALARS + sizeof(cjs_bz_tally) * std::min<uint64_t>(cap, ti.n_groups)));
  return 0;
}

}  // namespace

extern "C" int cjs_bzip2_tally(const uint8_t* in, size_t n, const cjs_bz_index* idx, const cjs_bz_lines* lines, uint64_t first, uint64_t count, uint64_t seed,
                               uint32_t mode, uint32_t delim, const cjs_cut_range* sel, uint32_t nsel, uint32_t order, uint64_t min_count, uint64_t max_count,
                               cjs_bz_tally* out, size_t cap, cjs_bz_tally_info* info, const cjs_opts* opts) {
  CJS_GUARD_BEGIN
  if (!in && n) return CJS_E_INVALID_ARG;
  return tally_core(in ? in : (const uint8_t*)"", nullptr, n, idx, lines, first, count, seed, mode, delim, sel, nsel, order, min_count, max_count, out, cap, info, opts,
                    TL_MAX_KEYS);
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

extern "C" int cjs_bzip2_tally_device(const uint8_t* d_in, size_t n, const cjs_bz_index* idx, const cjs_bz_lines* lines, uint64_t first, uint64_t count, uint64_t seed,
                                      uint32_t mode, uint32_t delim, const cjs_cut_range* sel, uint32_t nsel, uint32_t order, uint64_t min_count,
                                      uint64_t max_count, cjs_bz_tally* out, size_t cap, cjs_bz_tally_info* info, const cjs_opts* opts) {
  CJS_GUARD_BEGIN
  if (!d_in && n) return CJS_E_INVALID_ARG;
  return tally_core(nullptr, d_in, n, idx, lines, first, count, seed, mode, delim, sel, nsel, order, min_count, max_count, out, cap, info, opts, TL_MAX_KEYS);
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

// EXISTS FOR TESTS: the whole-line tally with the limit on the window's lines as an argument (no table of 2^32 lines fits a test).
// Exactly one of in / d_in.
extern "C" int cjs_stage_bzip2_tally_limit(const uint8_t* in, const uint8_t* d_in, size_t n, const cjs_bz_index* idx, const cjs_bz_lines* lines, uint64_t first,
                                           uint64_t count, uint64_t max_lines, cjs_bz_tally* out, size_t cap, cjs_bz_tally_info* info, const cjs_opts* opts) {
  CJS_GUARD_BEGIN
  if ((in != nullptr) == (d_in != nullptr)) return CJS_E_INVALID_ARG;
  return tally_core(in, d_in, n, idx, lines, first, count, 0, CJS_TALLY_LINES, 0, nullptr, 0, CJS_TALLY_BY_COUNT, 1, 0, out, cap, info, opts, max_lines);
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}
