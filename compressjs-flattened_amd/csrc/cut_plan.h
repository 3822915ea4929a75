// cut_plan.h -- the arithmetic of the column cut (cjs_bzip2_cut) as cut.hip computes it in pieces.  No HIP: the
// kernels and the host compiler read the same functions (tests/host/cut_plan_check.cc checks them against naive restatements).
//   A UNIT of a line is a field (fields mode: the delimiters in front of a byte, plus one) or a byte position (bytes mode), from 1.
//   The SELECTION is a sorted list of disjoint closed ranges of units; units 1 .. 64 are also a bit mask.
//   The STATE in front of a byte is (line number, units counted so far in its line, whether its line has a byte yet).  A piece of
//   text has a SUMMARY (newlines in it; units and "any byte" behind its last newline, or in all of it if it has none), summaries
//   compose (ct_comb, associative), and a state is the summary of everything in front of it with the line number for the newline
//   count: the state behind a piece is ct_comb(state in front, the piece's summary).  So a tile, a thread's share of it, a block and
//   a batch each get their carry-in from a scan of summaries, and the emit rule (ct_step) needs nothing but the state and the byte.
//   The unit counter saturates at CT_SAT: every further unit of such a line keeps the last number.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "cjs_hip.h"

#if defined(__HIPCC__)
#define CT_FN __host__ __device__ __forceinline__
#else
#define CT_FN inline
#endif

namespace cjs {

constexpr uint32_t CT_MAX_RANGES = 64, CT_SAT = 0xFFFFFFFEu, CT_TO_END = 0xFFFFFFFFu;
constexpr uint32_t CT_HAS_NL = 1u, CT_ANY = 2u;

// ---------------------------------------------------------------- the selection
// "1,3-5,7-", "-4": items N, N-M, N-, -M separated by commas.  0 or CJS_E_INVALID_ARG (cjs_hip.h lists the refusals).
inline int ct_parse_list(const char* list, cjs_cut_range* sel, uint32_t cap, uint32_t* nsel) {
  if (!list || !nsel || (!sel && cap)) return CJS_E_INVALID_ARG;
  uint32_t n = 0;
  const char* p = list;
  auto number = [&](uint32_t& v) {      // digits at p -> v; false for none, a zero or a value above CT_SAT
    if (*p < '0' || *p > '9') return false;
    uint64_t x = 0;
    for (; *p >= '0' && *p <= '9'; p++) { x = x * 10 + (uint64_t)(*p - '0'); if (x > CT_SAT) return false; }
    v = (uint32_t)x;
    return x != 0;
  };
  for (;;) {
    cjs_cut_range r{1, CT_TO_END};
    if (*p == '-') {                                   // -M
      p++;
      if (!number(r.hi)) return CJS_E_INVALID_ARG;
    } else {
      if (!number(r.lo)) return CJS_E_INVALID_ARG;
      if (*p == '-') {                                 // N- or N-M
        p++;
        if (*p != ',' && *p != 0 && !number(r.hi)) return CJS_E_INVALID_ARG;
      } else r.hi = r.lo;
    }
    if (r.lo > r.hi || n >= cap) return CJS_E_INVALID_ARG;
    sel[n++] = r;
    if (*p == 0) break;
    if (*p != ',') return CJS_E_INVALID_ARG;
    p++;
  }
  *nsel = n;
  return 0;
}

// The normalised selection: r[0 .. n) sorted, disjoint and not adjacent; mask bit k - 1 = unit k <= 64 is selected; r[beyond .. n)
// are the ranges that reach past unit 64; min_lo = the lowest selected unit.
struct CtSel {
  uint64_t mask;
  uint32_t mode, delim, n, beyond, min_lo, pad;
  cjs_cut_range r[CT_MAX_RANGES];
};

// The checks of the call's selection arguments and the normal form.  0 or CJS_E_INVALID_ARG.
inline int ct_normalise(uint32_t mode, uint32_t delim, const cjs_cut_range* sel, uint32_t nsel, CtSel* S) {
  if (mode != CJS_CUT_FIELDS && mode != CJS_CUT_BYTES) return CJS_E_INVALID_ARG;
  if (delim > 255 || (mode == CJS_CUT_FIELDS && delim == 0x0A)) return CJS_E_INVALID_ARG;
  if (!sel || nsel == 0 || nsel > CT_MAX_RANGES) return CJS_E_INVALID_ARG;
  for (uint32_t i = 0; i < nsel; i++) if (sel[i].lo == 0 || sel[i].lo > sel[i].hi) return CJS_E_INVALID_ARG;
  cjs_cut_range t[CT_MAX_RANGES];
  for (uint32_t i = 0; i < nsel; i++) {                // insertion sort by lo
    uint32_t j = i;
    for (; j > 0 && t[j - 1].lo > sel[i].lo; j--) t[j] = t[j - 1];
    t[j] = sel[i];
  }
  S->mode = mode; S->delim = delim; S->n = 0; S->mask = 0; S->pad = 0;
  for (uint32_t i = 0; i < nsel; i++) {                // merge what overlaps or touches
    if (S->n && (S->r[S->n - 1].hi == CT_TO_END || t[i].lo <= S->r[S->n - 1].hi + 1)) {
      if (t[i].hi > S->r[S->n - 1].hi) S->r[S->n - 1].hi = t[i].hi;
    } else S->r[S->n++] = t[i];
  }
  for (uint32_t i = S->n; i < CT_MAX_RANGES; i++) S->r[i] = cjs_cut_range{0, 0};
  S->min_lo = S->r[0].lo;
  S->beyond = S->n;
  for (uint32_t i = 0; i < S->n; i++) {
    const cjs_cut_range q = S->r[i];
    if (q.hi > 64 && S->beyond == S->n) S->beyond = i;
    if (q.lo > 64) continue;
    const uint32_t hi = q.hi < 64 ? q.hi : 64, w = hi - q.lo + 1;
    S->mask |= (w == 64 ? ~0ull : ((1ull << w) - 1)) << (q.lo - 1);
  }
  return 0;
}

// What the kernels and the walk read of a selection: the scalars by value, the ranges past unit 64 by pointer.
struct CtView {
  uint64_t mask;
  uint32_t mode, delim, min_lo, nbeyond;
  const cjs_cut_range* beyond;
};
inline CtView ct_view(const CtSel& S) { return CtView{S.mask, S.mode, S.delim, S.min_lo, S.n - S.beyond, S.r + S.beyond}; }

// unit k >= 1 is selected
CT_FN bool ct_member(const CtView& V, uint32_t k) {
  if (k <= 64) return (V.mask >> (k - 1)) & 1u;
  for (uint32_t i = 0; i < V.nbeyond; i++) {
    const cjs_cut_range q = V.beyond[i];
    if (k < q.lo) return false;
    if (k <= q.hi) return true;
  }
  return false;
}

// ---------------------------------------------------------------- summaries and states
// A summary: nl newlines; `units` counted and CT_ANY (any byte) behind the last of them, or in the whole piece without CT_HAS_NL.
// A state is the summary of the text in front of a byte, nl being the byte's line number.
struct CtSum { uint64_t nl; uint32_t units, flags; };
CT_FN CtSum ct_none() { return CtSum{0, 0, 0}; }
CT_FN uint32_t ct_sat_add(uint32_t a, uint32_t b) { const uint64_t s = (uint64_t)a + b; return s > CT_SAT ? CT_SAT : (uint32_t)s; }
// a, then b
CT_FN CtSum ct_comb(const CtSum& a, const CtSum& b) {
  if (b.flags & CT_HAS_NL) return CtSum{a.nl + b.nl, b.units, b.flags};
  return CtSum{a.nl + b.nl, ct_sat_add(a.units, b.units), a.flags | b.flags};
}
// s, then byte ch
CT_FN void ct_push(CtSum& s, uint32_t mode, uint32_t delim, uint8_t ch) {
  if (ch == 0x0A) { s.nl++; s.units = 0; s.flags = CT_HAS_NL; return; }
  s.flags |= CT_ANY;
  if ((mode == CJS_CUT_BYTES || ch == delim) && s.units < CT_SAT) s.units++;
}
inline CtSum ct_summary(const uint8_t* text, size_t n, uint32_t mode, uint32_t delim) {
  CtSum s = ct_none();
  for (size_t i = 0; i < n; i++) ct_push(s, mode, delim, text[i]);
  return s;
}

// The emit rule: is byte ch, met in state s, written when the window is lines [first, end)?  s becomes the state behind it.
CT_FN bool ct_step(const CtView& V, uint64_t first, uint64_t end, CtSum& s, uint8_t ch) {
  const bool in = s.nl >= first && s.nl < end;
  if (ch == 0x0A) { s.nl++; s.units = 0; s.flags = CT_HAS_NL; return in; }
  s.flags |= CT_ANY;
  if (V.mode == CJS_CUT_FIELDS) {
    if (ch != V.delim) return in && ct_member(V, s.units + 1);
    if (s.units < CT_SAT) s.units++;
    const uint32_t k = s.units + 1;                    // the field this delimiter opens
    return in && k > V.min_lo && ct_member(V, k);
  }
  const uint32_t k = s.units + 1;
  if (s.units < CT_SAT) s.units++;
  return in && ct_member(V, k);
}

// A piece of text met in state s: out gets the first min(cap, written) of the bytes it writes; returns their number.
inline size_t ct_piece(const CtView& V, uint64_t first, uint64_t end, CtSum& s, const uint8_t* text, size_t n, uint8_t* out, size_t cap) {
  size_t w = 0;
  for (size_t i = 0; i < n; i++)
    if (ct_step(V, first, end, s, text[i])) { if (w < cap) out[w] = text[i]; w++; }
  return w;
}
// the newline a tail line gets: state s stands behind the last byte of the text
CT_FN bool ct_tail_newline(const CtSum& s, uint64_t first, uint64_t end) { return (s.flags & CT_ANY) && s.nl >= first && s.nl < end; }

// The scalar walk behind cjs_stage_cut: all lines of text[0 .. n).  Returns the full size; out gets the first min(cap, size) bytes.
inline size_t cut_text(const CtSel& S, const uint8_t* text, size_t n, uint8_t* out, size_t cap) {
  const CtView V = ct_view(S);
  CtSum s = ct_none();
  size_t w = ct_piece(V, 0, ~0ull, s, text, n, out, cap);
  if (ct_tail_newline(s, 0, ~0ull)) { if (w < cap) out[w] = 0x0A; w++; }
  return w;
}

}  // namespace cjs
