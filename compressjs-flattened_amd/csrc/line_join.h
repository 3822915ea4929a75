// line_join.h -- the host half of a key pass (linekeys.hip): what the kernels and the host hand each other per block,
// the layout of a pass's workspace, and the join of the blocks' fragments into the keys of a window's lines.  No HIP in here
// (tests/host/line_join_check.cc runs the join over random texts, blocks and windows with the host compiler).
#pragma once
#include "bz_lines.h"
#include "line_key.h"
#include "tally_plan.h"      // tl_join_newline: the tally's rule for the tail line
#include <string.h>
#include <algorithm>
#include <vector>

namespace cjs {

constexpr uint32_t LK_TILE = 16384;                        // bytes of a tile: that of the line table
struct LkBlk { uint64_t src, rec0; uint32_t len, tile0, nrec, blk; };      // len bytes at src; its records from rec0 on, nrec of them by the table
struct LkOpen { uint64_t h1, h2; uint32_t len, has; };                     // a tile's open fragment (lk_summary), then its carry-in (lk_chain)
struct LkTail { uint64_t h1, h2, head_h2; uint32_t len, pad; };            // per block: the fragment behind its last newline; H_B2 of its first record in full
struct LkPatch { uint64_t at; cjs_bz_linekey key; };                       // keys[at] = key (lk_patch; no `at` twice)

LK_FN uint32_t lk_tiles(uint32_t len) { return (len + LK_TILE - 1) / LK_TILE; }

// A pass's workspace over nblk blocks (or pieces of text) in nt tiles: the offsets of its arrays and their sum.  nrec: the records
// kept in the pass's own memory (0: lk_emit writes into the caller's array); heads: room for a block's first record (lk_heads).
struct LkLayout {
  size_t blk = 0, cnt, open, tot, tail, rec, head, bytes;
  static size_t pad(size_t x) { return (x + 255) & ~(size_t)255; }
  LkLayout(size_t nblk, size_t nt, size_t nrec, bool heads) {
    cnt = blk + pad(sizeof(LkBlk) * nblk); open = cnt + pad(4 * nt); tot = open + pad(sizeof(LkOpen) * nt); tail = tot + pad(4 * nblk);
    rec = tail + pad(sizeof(LkTail) * nblk); head = rec + pad(sizeof(cjs_bz_linekey) * nrec); bytes = head + (heads ? pad(sizeof(cjs_bz_linekey) * nblk) : 0);
  }
};
struct LkMem {                                             // ... and the arrays themselves, in `bytes` bytes at d
  LkBlk* blk; uint32_t* cnt; LkOpen* open; uint32_t* tot; LkTail* tail; cjs_bz_linekey *rec, *head;
  LkMem(uint8_t* d, const LkLayout& L) : blk((LkBlk*)(d + L.blk)), cnt((uint32_t*)(d + L.cnt)), open((LkOpen*)(d + L.open)), tot((uint32_t*)(d + L.tot)),
                                         tail((LkTail*)(d + L.tail)), rec((cjs_bz_linekey*)(d + L.rec)), head((cjs_bz_linekey*)(d + L.head)) {}
};

// The keys of plain text in device memory (text_keys_device) cut it into pieces of `piece` bytes, LK_PIECE outside tests; its
// workspace holds a pass over the pieces, their records in the caller's array, and a patch per piece and the tail behind it.
constexpr size_t LK_PIECE = 900000;
inline size_t text_keys_pieces(size_t n, size_t piece) { return (n + piece - 1) / piece; }
inline size_t text_keys_work_bytes(size_t n, size_t piece) {
  const size_t np = text_keys_pieces(n, piece), nt = n / LK_TILE + np + 1;      // (no fewer than the pieces' tiles)
  return LkLayout(np, nt, 0, true).bytes + LkLayout::pad(sizeof(LkPatch) * (np + 1)) + 256;
}

// The fragments of the touched blocks, as they come, joined into the keys of the window's lines.
struct LkJoin {
  const cjs_bz_lines* t = nullptr;
  LkBases B{0, 0};
  uint64_t first = 0, end = 0;                              // the window
  cjs_bz_linekey* keys = nullptr; size_t cap = 0;
  const std::vector<uint32_t>* touched = nullptr; size_t at = 0;      // touched blocks in front of `at` are done
  LkFrag open{0, 0, 0}; bool open_bad = false;              // the line that stands open behind the blocks so far
  // The tally's destination: a device array of the window's lines (cap = all of them).  The whole-line records of a block go there
  // from the batch (LineKeysCall); what the join makes is kept here and goes up at the end: the patches (at most one per touched
  // block and the tail), and the lines of the bad blocks as ranges to fill with all-ones.
  cjs_bz_linekey* d_keys = nullptr;
  std::vector<LkPatch> patches; std::vector<std::pair<uint64_t, uint64_t>> fills;
  bool tally_tail = true;                                   // with d_keys: the tally's rule for the tail line (finish), or the plain one
  bool tail_dropped = false;                                // the tally's tail rule found the tail line empty: it is no line

  void put(uint64_t line, const cjs_bz_linekey& k) {
    if (line < first || line >= end || line - first >= cap) return;
    if (d_keys) patches.push_back(LkPatch{line - first, k}); else keys[line - first] = k;
  }
  // a touched block that did not come as a good one: its lines, the one that goes on behind it included
  void bad(uint32_t b) {
    if (d_keys) {
      const uint64_t lo = std::max<uint64_t>(t->cum[b], first), hi = std::min<uint64_t>(t->cum[b + 1], end);      // (the line behind them: by open_bad)
      if (lo < hi) fills.emplace_back(lo - first, hi - first);
    } else for (uint64_t k = t->cum[b]; k < t->cum[b + 1]; k++) put(k, lk_bad_key());
    open = LkFrag{0, 0, 0}; open_bad = true;
  }
  void good(uint32_t b, const cjs_bz_linekey* recs, const LkTail& tail) {
    while (at < touched->size() && (*touched)[at] < b) bad((*touched)[at++]);
    at++;
    const LkFrag behind{tail.h1, tail.h2, tail.len};
    const uint32_t n = t->nl[b];
    if (!n) { open = lk_join(open, behind, B); return; }      // no newline: the whole block goes on the open line
    const uint64_t l0 = t->cum[b];
    put(l0, open_bad ? lk_bad_key() : lk_key(lk_join(open, LkFrag{recs[0].hash, tail.head_h2, recs[0].len}, B)));
    // the others stand whole in the block: their records are their keys
    const uint64_t lo = std::max<uint64_t>(l0 + 1, first), hi = std::min<uint64_t>(std::min<uint64_t>(l0 + n, end), first + cap);
    if (lo < hi && !d_keys) memcpy(keys + (lo - first), recs + (lo - l0), sizeof(cjs_bz_linekey) * (size_t)(hi - lo));      // (d_keys: the batch has copied them)
    open = behind; open_bad = false;
  }
  void finish() {
    while (at < touched->size()) bad((*touched)[at++]);
    const uint64_t tail = t->cum.back();                             // the tail line (inside the window iff the last block was touched)
    if (!d_keys || !tally_tail) { put(tail, open_bad ? lk_bad_key() : lk_key(open)); return; }
    // the tally's rule for the tail: an empty one is no line, any other is keyed as if it ended in a newline
    if (tail < first || tail >= end) return;
    if (open_bad) put(tail, lk_bad_key());
    else if (open.len == 0) tail_dropped = true;
    else put(tail, lk_key(tl_join_newline(open, B)));
  }
};

}  // namespace cjs
