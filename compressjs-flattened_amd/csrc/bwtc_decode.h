// bwtc_decode.h — the serial entropy stage of BWTC.decompressFile (J/BWTC_joined_.js:1827-1920): a parser of UNTRUSTED bytes.
// Range decoding and the adaptive model are one serial chain over the whole file (every decoded symbol feeds the
// model that decodes the next one), so that part runs on one host thread; the inverse BWT of all blocks
// (BWT.unbwtransform, n dependent gathers per block in the reference) runs on the GPU (dec_ibwt.hip).
//
// The host side keeps the stream format's arithmetic (it IS the format) but not the reference's data structures: the
// adaptive models are flat per-symbol counters laid out in CODING ORDER with 16-entry bucket sums, searched linearly
// (2 short scans per symbol), instead of the reference's implicit binary tree walked and updated level by level.
// No HIP in here (tests/host/bwtc_host_check.cc compiles it with the host compiler and feeds it damaged streams under the
// sanitizers).
#pragma once
#include "bwtc_format.h"
#include "cjs_hip.h"
#include <stddef.h>
#include <stdio.h>
#include <string.h>
#include <optional>
#include <vector>

namespace cjs {
namespace {      // internal linkage, as when this stood in bwtc.hip: the library exports none of it

// Byte source + the decoder half of the carry-less range coder (interval state as RangeCoder's decode side, :159-238).
class RangeDecoder {
 public:
  RangeDecoder(const uint8_t* p, size_t n, size_t at) : in_(p), n_(n), pos_(at) {}
  void begin() { last_ = next_byte(); low_ = (uint32_t)last_ >> 1; range_ = 1u << 7; }           // decodeStart(skipInitialRead)
  // cumulative-frequency target under total `tot` / under 2^sh; the matching commit() must follow
  uint32_t target(uint32_t tot) { refill(); unit_ = range_ / tot; const uint32_t t = unit_ ? low_ / unit_ : 0; return t >= tot ? tot - 1 : t; }
  uint32_t target_pow2(int sh) { refill(); unit_ = range_ >> sh; const uint32_t t = unit_ ? low_ / unit_ : 0; return (t >> sh) ? (1u << sh) - 1 : t; }
  void commit(uint32_t sy, uint32_t lt, uint32_t tot) { const uint32_t base = unit_ * lt; low_ -= base; if (lt + sy < tot) range_ = unit_ * sy; else range_ -= base; }
  uint32_t bit() { const uint32_t t = target_pow2(1); commit(1, t, 2); return t; }
  uint32_t bits(int k) { uint32_t r = 0; while (k-- > 0) r = (r << 1) | bit(); return r; }         // NoModel (:1274-1287)
  uint32_t log_distance(int block_size) {                                                           // LogDistanceModel.decode (:1254-1261)
    const uint32_t lg = bits(lgbits(block_size));
    return lg < 2 ? lg : (1u << (lg - 1)) + bits((int)lg - 1);
  }
  bool exhausted() const { return past_end_ > 8; }       // a well-formed stream never reads more than a few bytes past its end
  size_t consumed() const { return pos_; }
 private:
  int32_t next_byte() { if (pos_ < n_) return in_[pos_++]; past_end_++; return -1; }
  void refill() {
    while (range_ <= 0x00800000u) {
      low_ = (low_ << 8) | (((uint32_t)last_ << 7) & 0xFF);
      last_ = next_byte();
      low_ |= (uint32_t)last_ >> 1;
      range_ <<= 8;
    }
  }
  const uint8_t* in_; size_t n_, pos_;
  uint32_t low_ = 0, range_ = 0, unit_ = 0, past_end_ = 0; int32_t last_ = 0;
};

// FenwickModel, decode side (:1572-1661), as flat counters.  The reference keeps (count << 16 | unseen marker) in an
// implicit binary tree over num_syms leaves (num_syms not a power of two): the cumulative order of the symbols is the
// left-to-right order of the leaves = the deepest level first.  Here: slot o of the coding order holds the count and the
// unseen marker of symbol sym_[o]; 16-slot bucket sums make the cumulative search two short linear scans.
class RankModelDecoder {
 public:
  RankModelDecoder(RangeDecoder& d, int size) : d_(d), n_(size + 1) {
    int deep = 1; while (deep * 2 <= 2 * n_ - 1) deep *= 2;          // first heap position of the deepest level
    int o = 0;
    for (int leaf = deep; leaf < 2 * n_; leaf++) sym_[o++] = (uint16_t)(leaf - n_);
    for (int leaf = n_; leaf < deep; leaf++) sym_[o++] = (uint16_t)(leaf - n_);
    for (o = 0; o < n_; o++) { const bool esc = sym_[o] == n_ - 1; cnt_[o] = esc ? 0x100u : 0u; unseen_[o] = esc ? 0 : 1; if (esc) esc_slot_ = o; }
    resum();
  }
  int decode() {                                                    // -1: corrupt stream
    int o = take(cnt_, bcnt_, cnt_total_);
    if (o < 0) return -1;
    if (o == esc_slot_) {
      // the escape symbol: the novel symbol follows in the distribution of the unseen markers (:1590-1600); once the
      // last unseen symbol is about to go the escape symbol disappears with it (:1648)
      cnt_[o] += 0x100u; bcnt_[o >> 4] += 0x100u; cnt_total_ += 0x100u;
      if (unseen_total_ == 1) { cnt_total_ -= cnt_[o]; bcnt_[o >> 4] -= cnt_[o]; cnt_[o] = 0; }
      if (cnt_total_ >= 0xFF00u) halve();
      uint32_t ut = unseen_total_;
      if (ut == 0) return -1;
      o = take_unseen(ut);
      if (o < 0) return -1;
      unseen_[o] = 0; bun_[o >> 4]--; unseen_total_--;
    }
    cnt_[o] += 0x100u; bcnt_[o >> 4] += 0x100u; cnt_total_ += 0x100u;
    if (cnt_total_ >= 0xFF00u) halve();
    return sym_[o];
  }
 private:
  // slot whose cumulative count interval holds the coder's target; commits the step with the count BEFORE the update
  int take(const uint32_t* c, const uint32_t* bc, uint32_t tot) {
    if (tot == 0) return -1;
    const uint32_t t = d_.target(tot);
    uint32_t lt = 0; int b = 0;
    const int nbuck = (n_ + 15) >> 4;
    while (b < nbuck - 1 && lt + bc[b] <= t) lt += bc[b++];
    int o = b << 4;
    while (o < n_ - 1 && lt + c[o] <= t) lt += c[o++];
    d_.commit(c[o], lt, tot);
    return o;
  }
  int take_unseen(uint32_t tot) {
    const uint32_t t = d_.target(tot);
    uint32_t lt = 0; int b = 0;
    const int nbuck = (n_ + 15) >> 4;
    while (b < nbuck - 1 && lt + bun_[b] <= t) lt += bun_[b++];
    int o = b << 4;
    while (o < n_ - 1 && lt + unseen_[o] <= t) lt += unseen_[o++];
    d_.commit(unseen_[o], lt, tot);
    return unseen_[o] ? o : -1;
  }
  void halve() {                                                    // rescale (:1623-1646)
    bool any_unseen = false;
    for (int o = 0; o < n_; o++) {
      if (o == esc_slot_) continue;
      if (unseen_[o]) { any_unseen = true; continue; }
      cnt_[o] >>= 1;
      if (cnt_[o] == 0) { unseen_[o] = 1; any_unseen = true; }      // a count that halves to nothing makes the symbol novel again
    }
    uint32_t e = cnt_[esc_slot_] >> 1;
    cnt_[esc_slot_] = any_unseen ? (e ? e : 1u) : 0u;
    resum();
  }
  void resum() {
    const int nbuck = (n_ + 15) >> 4;
    cnt_total_ = unseen_total_ = 0;
    for (int b = 0; b < nbuck; b++) bcnt_[b] = bun_[b] = 0;
    for (int o = 0; o < n_; o++) { bcnt_[o >> 4] += cnt_[o]; bun_[o >> 4] += unseen_[o]; cnt_total_ += cnt_[o]; unseen_total_ += unseen_[o]; }
  }
  RangeDecoder& d_;
  int n_, esc_slot_ = 0;                                            // n_ = coded symbols incl. the escape symbol (the last one)
  uint16_t sym_[272];
  uint32_t cnt_[272], unseen_[272], bcnt_[17], bun_[17];
  uint32_t cnt_total_ = 0, unseen_total_ = 0;
};

// DefSumModel, decode side (:1327-1459): 8-bit total, counts folded in only every `quota_` symbols.  Lookup of the symbol
// from the 8-bit target is a direct 256-entry table rebuilt at every fold; the escape distribution is uniform over the
// symbols whose count is still zero.
class DeferredSumDecoder {
 public:
  DeferredSumDecoder(RangeDecoder& d, int size) : d_(d), esc_(size) {
    memset(cum_, 0, sizeof cum_); memset(pend_, 0, sizeof pend_);
    cum_[esc_ + 1] = 256;                                           // everything on the escape symbol at first
    for (int i = 0; i <= esc_; i++) zero_rank_[i] = (uint16_t)i;
    for (int i = 0; i < 256; i++) by_target_[i] = (uint16_t)esc_;
    for (int i = 0; i < 304; i++) by_zero_rank_[i] = (uint16_t)(i < esc_ ? i : 0);
  }
  int decode() {
    int sym = by_target_[d_.target_pow2(8)];
    d_.commit((uint32_t)cum_[sym + 1] - cum_[sym], cum_[sym], 256);
    note(sym);
    if (sym != esc_) return sym;
    const uint32_t nzero = zero_rank_[esc_];
    if (nzero == 0) return -1;
    sym = by_zero_rank_[d_.target(nzero)];
    d_.commit((uint32_t)zero_rank_[sym + 1] - zero_rank_[sym], zero_rank_[sym], nzero);
    note(sym);
    return sym;
  }
 private:
  void note(int sym) {                                              // :1398-1429
    if (sym == esc_ && (pend_[sym] >= 40 || seen_ >= quota_ - 1)) return;
    pend_[sym]++; seen_++;
    if (seen_ < quota_) return;
    int total = 0, zeros = 0, odd = 0;
    for (int i = 0; i <= esc_; i++) {                               // halve the old share, add what arrived since
      const int c = ((cum_[i + 1] - cum_[i]) >> 1) + pend_[i];
      cum_[i] = (uint16_t)total; zero_rank_[i] = (uint16_t)zeros;
      if (c) { total += c; odd += c & 1; } else zeros++;
    }
    cum_[esc_ + 1] = (uint16_t)total;
    quota_ = 256 - (total - odd) / 2;
    memset(pend_, 0, sizeof pend_);
    pend_[esc_] = 1; seen_ = 1;
    int t = 0, z = 0;
    for (int i = 0; i <= esc_; i++) {
      for (; t < cum_[i + 1]; t++) by_target_[t] = (uint16_t)i;
      const int ze = i + 1 <= esc_ ? zero_rank_[i + 1] : 0;         // the reference's escape[] has esc_+1 entries
      for (; z < ze; z++) by_zero_rank_[z] = (uint16_t)i;
    }
  }
  RangeDecoder& d_;
  int esc_;                                                         // number of ordinary symbols = index of the escape symbol
  uint16_t cum_[304], zero_rank_[304], pend_[304], by_target_[256], by_zero_rank_[304];
  int seen_ = 0, quota_ = 128;
};

struct BwtcBlocks {                     // output of the serial stage: the BWT columns of all blocks, back to back
  std::vector<uint8_t> cols;
  std::vector<uint32_t> lens, pidx;
  int level = 0;
};

// header, per-block flag / length / primary index / use-tree, symbol decode, RLE2 + MTF inverse (:1827-1913).  dbg: one line
// per block on stderr (CJS_DEBUG)
inline int bwtc_entropy_decode(const uint8_t* in, size_t n, BwtcBlocks& B, bool dbg) {
  if (n < 4 || in[0] != 'b' || in[1] != 'w' || in[2] != 't' || in[3] != 'c') return CJS_E_BAD_MAGIC;     // :559-565
  size_t p = 4;
  for (;;) { if (p >= n) return CJS_E_DATA_ERROR; if (in[p++] & 0x80) break; }                          // readUnsignedNumber :621-633
  RangeDecoder d(in, n, p);
  d.begin();
  const uint32_t lv = d.target_pow2(8); d.commit(1, lv, 256);                                          // decodeByte :1830
  if (lv < 1 || lv > 9) return CJS_E_DATA_ERROR;
  B.level = (int)lv;
  const bool fast = lv <= 5;
  const uint32_t bs = lv * 100000u;
  for (;;) {
    const uint32_t flag = d.target(3); d.commit(1, flag, 3);
    uint32_t length;
    if (flag == 0) length = bs;
    else if (flag == 1) { length = d.log_distance((int)bs); if (length > bs) return CJS_E_DATA_ERROR; }
    else break;
    const uint32_t pi = d.log_distance((int)bs);
    uint16_t tree[512]; memset(tree, 0, sizeof tree); tree[0] = 1;                                     // use-tree :1859-1874
    for (int i = 1; i < 512; i++) {
      const int parent = i >> 1, full = use_tree_full(i);
      if (tree[parent] == 0 || tree[parent] == full * 2) tree[i] = tree[parent] >> 1;
      else if (i >= 256) tree[i] = (uint16_t)d.bit();
      else { const uint32_t v = d.target(3); d.commit(1, v, 3); tree[i] = (uint16_t)(v == 2 ? (uint32_t)full : v); }
    }
    uint8_t order[256]; int asz = 0;
    for (int i = 0; i < 256; i++) if (tree[256 + i]) order[asz++] = (uint8_t)i;
    if (d.exhausted()) return CJS_E_DATA_ERROR;
    // the block is stored at its decoded length (a forged header cannot make the host reserve a full block per 13 bits)
    const size_t base = B.cols.size();
    B.cols.resize(base + length);
    uint8_t* b = B.cols.data() + base;
    uint64_t run = 1; uint32_t i = 0; bool bad = false;
    {
      std::optional<RankModelDecoder> rm; std::optional<DeferredSumDecoder> dm;
      if (fast) dm.emplace(d, asz + 1); else rm.emplace(d, asz + 1);
      while (i < length) {                                                                             // :1888-1903
        const int c = fast ? dm->decode() : rm->decode();
        if (c < 0 || d.exhausted()) { bad = true; break; }
        if (c <= 1) {                                                // RUNA / RUNB: bijective base-2 digits of a zero run
          const uint64_t add = run << c;
          if (i + add > length) { bad = true; break; }
          memset(b + i, 0, (size_t)add); i += (uint32_t)add; run *= 2;
        } else { run = 1; if (c - 1 >= asz) { bad = true; break; } b[i++] = (uint8_t)(c - 1); }
      }
    }
    if (dbg) fprintf(stderr, "[cjs bwtc dec] block %zu: length %u pidx %u asz %d decoded %u bad %d inpos %zu/%zu\n", B.lens.size(), length, pi, asz, i, (int)bad, d.consumed(), n);
    if (bad || pi > length) return CJS_E_DATA_ERROR;
    for (i = 0; i < length; i++) {                                                                     // MTF decode :1905-1913
      const int j = b[i]; const uint8_t c = order[j];
      b[i] = c;
      if (j) { memmove(order + 1, order, (size_t)j); order[0] = c; }
    }
    if (length == 0) { B.cols.resize(base); continue; }             // an empty block contributes nothing (unbwtransform of 0 bytes)
    B.lens.push_back(length); B.pidx.push_back(pi);
  }
  return 0;
}

}  // namespace
}  // namespace cjs
