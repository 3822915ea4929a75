// line_diff.h -- the line diff of two key lists (cjs_line_keys_diff): a shortest edit script as hunks.  No HIP and
// no device: plain arrays of cjs_bz_linekey (tests/host/line_key_check.cc checks it against the quadratic DP).
// The common prefix and suffix are trimmed; the rest goes through Myers' O(ND) search with the linear-space middle-snake
// recursion: the two furthest-reaching frontiers, forwards and backwards, are all that is kept (O(max_edits) words), no trace.
// Every level of the recursion trims again, so a sub-problem with one side empty is an insertion or a deletion, and one with both
// sides non-empty needs at least two edits: both halves of its split are strictly smaller.
#pragma once
#include "line_key.h"
#include <algorithm>
#include <vector>

namespace cjs {

constexpr uint64_t LK_DIFF_DEFAULT_MAX_EDITS = 16384;      // (an unmeasured choice: 16 K edits are a frontier of 256 KiB)

// The hunks as they come, ascending: edits that touch are one hunk, a common line in between closes it.
struct LkHunks {
  cjs_bz_hunk* out; size_t cap; uint64_t n = 0, edits = 0;
  cjs_bz_hunk cur{0, 0, 0, 0}; bool open = false;
  LkHunks(cjs_bz_hunk* o, size_t c) : out(o), cap(c) {}
  void edit(uint64_t a_pos, uint64_t a_cnt, uint64_t b_pos, uint64_t b_cnt) {
    if (!(a_cnt | b_cnt)) return;
    edits += a_cnt + b_cnt;
    if (open && cur.a_first + cur.a_count == a_pos && cur.b_first + cur.b_count == b_pos) { cur.a_count += a_cnt; cur.b_count += b_cnt; return; }
    flush();
    cur = cjs_bz_hunk{a_pos, a_cnt, b_pos, b_cnt}; open = true;
  }
  void flush() {
    if (!open) return;
    if (n < cap) out[n] = cur;
    n++; open = false;
  }
};

struct LkDiff {
  const cjs_bz_linekey* A; const cjs_bz_linekey* B;
  std::vector<int64_t> vf, vb;      // the frontiers: furthest x on diagonal k at index k + off
  int64_t off = 0, dmax = 0;
  LkHunks* H = nullptr;

  struct Snake { int64_t x, y, u, v; uint64_t edits; bool found; };
  // The middle snake of A[a0, a1) against B[b0, b1), both non-empty and without a common first or last line: the matching run
  // (x, y) .. (u, v) that a shortest script passes halfway, and that script's edits: the frontiers meet after D steps each, which
  // makes 2D - 1 (seen forwards) or 2D (seen backwards).  found = false: they did not meet within dmax steps.
  Snake middle(int64_t a0, int64_t a1, int64_t b0, int64_t b1) {
    const int64_t N = a1 - a0, M = b1 - b0, delta = N - M;
    const bool odd = (delta & 1) != 0;
    const int64_t dlim = std::min(dmax, (N + M + 1) / 2);
    int64_t* F = vf.data() + off; int64_t* R = vb.data() + off;
    F[1] = 0; R[1] = 0;
    for (int64_t D = 0; D <= dlim; D++) {
      for (int64_t k = -D; k <= D; k += 2) {
        int64_t x = (k == -D || (k != D && F[k - 1] < F[k + 1])) ? F[k + 1] : F[k - 1] + 1;
        int64_t y = x - k;
        const int64_t xs = x, ys = y;
        while (x < N && y < M && lk_same(A[a0 + x], B[b0 + y])) { x++; y++; }
        F[k] = x;
        const int64_t kr = delta - k;      // the same diagonal as the backward search numbers it
        if (odd && kr >= -(D - 1) && kr <= D - 1 && x + R[kr] >= N) return Snake{a0 + xs, b0 + ys, a0 + x, b0 + y, (uint64_t)(2 * D - 1), true};
      }
      for (int64_t k = -D; k <= D; k += 2) {
        int64_t x = (k == -D || (k != D && R[k - 1] < R[k + 1])) ? R[k + 1] : R[k - 1] + 1;
        int64_t y = x - k;
        const int64_t xs = x, ys = y;
        while (x < N && y < M && lk_same(A[a1 - 1 - x], B[b1 - 1 - y])) { x++; y++; }
        R[k] = x;
        const int64_t kf = delta - k;
        if (!odd && kf >= -D && kf <= D && x + F[kf] >= N) return Snake{a1 - x, b1 - y, a1 - xs, b1 - ys, (uint64_t)(2 * D), true};
      }
    }
    return Snake{0, 0, 0, 0, 0, false};
  }

  void trim(int64_t& a0, int64_t& a1, int64_t& b0, int64_t& b1) const {
    while (a0 < a1 && b0 < b1 && lk_same(A[a0], B[b0])) { a0++; b0++; }
    while (a0 < a1 && b0 < b1 && lk_same(A[a1 - 1], B[b1 - 1])) { a1--; b1--; }
  }
  void whole(int64_t a0, int64_t a1, int64_t b0, int64_t b1) { H->edit((uint64_t)a0, (uint64_t)(a1 - a0), (uint64_t)b0, (uint64_t)(b1 - b0)); }

  // The script of A[a0, a1) against B[b0, b1), in ascending order.  A sub-problem needs no more edits than the problem it is a
  // half of, so its frontiers meet; should they not, the range goes out as one replacement and the script is no longer minimal.
  void solve(int64_t a0, int64_t a1, int64_t b0, int64_t b1) {
    trim(a0, a1, b0, b1);
    if (a0 == a1 || b0 == b1) return whole(a0, a1, b0, b1);
    const Snake s = middle(a0, a1, b0, b1);
    if (!s.found) { minimal = false; return whole(a0, a1, b0, b1); }
    solve(a0, s.x, b0, s.y);
    solve(s.u, a1, s.v, b1);
  }
  bool minimal = true;
};

inline int lk_diff(const cjs_bz_linekey* a, size_t na, const cjs_bz_linekey* b, size_t nb, uint64_t max_edits, cjs_bz_hunk* hunks, size_t cap,
                   cjs_bz_ldiff_info* info) {
  if (!max_edits) max_edits = LK_DIFF_DEFAULT_MAX_EDITS;
  LkHunks H(hunks, cap);
  LkDiff D;
  D.A = a; D.B = b; D.H = &H;
  int64_t a0 = 0, a1 = (int64_t)na, b0 = 0, b1 = (int64_t)nb;
  D.trim(a0, a1, b0, b1);
  if (a0 == a1 || b0 == b1) {
    // an insertion or a deletion is the only shortest script, but it is held to the cap like any other
    D.minimal = (uint64_t)(a1 - a0) + (uint64_t)(b1 - b0) <= max_edits;
    D.whole(a0, a1, b0, b1);
  } else {
    // frontiers for scripts of up to max_edits edits: D <= max_edits / 2 + 1 steps, diagonals -D - 1 .. D + 1
    const uint64_t most = (uint64_t)(a1 - a0) + (uint64_t)(b1 - b0);
    D.dmax = (int64_t)(std::min(max_edits, most) / 2 + 1); D.off = D.dmax + 2;
    D.vf.assign((size_t)(2 * D.dmax + 5), 0); D.vb.assign((size_t)(2 * D.dmax + 5), 0);
    const LkDiff::Snake s = D.middle(a0, a1, b0, b1);
    if (s.found && s.edits <= max_edits) {
      D.solve(a0, s.x, b0, s.y);
      D.solve(s.u, a1, s.v, b1);
    } else {
      D.minimal = false;
      D.whole(a0, a1, b0, b1);
    }
  }
  H.flush();
  info->n_hunks = H.n; info->edits = H.edits; info->common = ((uint64_t)na + (uint64_t)nb - H.edits) / 2;
  info->minimal = D.minimal ? 1u : 0u; info->reserved = 0;
  return 0;
}

}  // namespace cjs
