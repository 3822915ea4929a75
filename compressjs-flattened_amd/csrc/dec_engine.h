// dec_engine.h -- the Bzip2 decode engine as its drivers see it.  Each phase is a file of its own, kernels and host steps together:
// dec_blocks.hip (phase A), dec_ibwt.hip (phase B), dec_unrle1.hip (phase C); decode.hip holds the header, level and verdict helpers
// and the single-stream driver bunzip_core.  The drivers in dec_batch.hip (host and device batch, device single), dec_recover.hip
// (recovery), range.hip (indexed range reads; search.hip runs on its pass engine) and dec_stream.hip (streaming) sit on what is
// declared here.
// The glue between the phases is written once: bz_header_check (_start_bunzip), WalkCands + walk_chain (candidate lookup, bz_walk,
// chain append), chain_out_offsets (the prefix sum), group_layout / group_prepare / group_verdicts (a batch group, both forms),
// dec_scratch_batches (phases B and C batch by batch into scratch: recovery and range reads), ShareScratch (a phase's own scratch).
// A driver holds what is particular to it: where the bytes come from and where they go.
#pragma once
#include "cjs_internal.h"
#include "bz_frame.h"
#include "decode_dev.h"
#include "host.h"
#include <algorithm>
#include <chrono>
#include <functional>
#include <string>
#include <vector>

namespace cjs {

struct IbBlock {            // per valid block, in stream order
  uint64_t tt;              // device address of the block's decoded BWT bytes
  uint32_t count;           // n
  uint32_t orig;
  uint32_t off;             // element offset of the block in the concatenated sort / LF arrays
  uint32_t woff;            // byte offset of the block in the walk's output (w)
  uint64_t out_off;         // byte offset of the block in the final output
  uint32_t out_len;
  uint32_t crc;
};
// a decoded block candidate, its BWT bytes at device address tt, as a chain block of phases B and C
inline IbBlock ib_block(const BlockOut& bo, uint64_t tt) {
  IbBlock ib; ib.tt = tt; ib.count = bo.count; ib.orig = bo.orig; ib.off = 0; ib.woff = 0; ib.out_off = 0; ib.out_len = 0; ib.crc = bo.crc;
  return ib;
}

constexpr uint32_t DEC_BATCH_BLOCKS = 65535;          // blocks of an inverse-BWT batch: grid.y of the per-block kernels

// Device scratch of one streaming decoder (cjs_bzip2_dec_*): ONE allocation made at the decoder's first step, handed out first fit
// in 256-byte units and taken back piece by piece, so what a decoder holds between its steps never changes.  A request that does
// not fit (the size is an estimate) becomes a hipMalloc of its own, freed when it is given back.
struct DecArena {
  DevMem<uint8_t> base; size_t cap = 0;
  std::vector<std::pair<size_t, size_t>> free_;      // (offset, bytes), ascending, coalesced
  std::vector<std::pair<void*, size_t>> used;        // bytes == 0: a hipMalloc of its own
  uint32_t spills = 0;
  int init(size_t bytes) { CJS_TRY(base.alloc(bytes)); cap = bytes; free_.assign(1, {0, bytes}); return 0; }
  void* take(size_t bytes) {
    bytes = (std::max<size_t>(bytes, 1) + 255) & ~(size_t)255;
    for (size_t i = 0; i < free_.size(); i++) if (free_[i].second >= bytes) {
      void* p = base.p + free_[i].first;
      if (free_[i].second == bytes) free_.erase(free_.begin() + (long)i); else { free_[i].first += bytes; free_[i].second -= bytes; }
      used.push_back({p, bytes});
      return p;
    }
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    spills++;
    used.push_back({p, 0});
    return p;
  }
  void give(void* p) {
    size_t i = 0;
    while (i < used.size() && used[i].first != p) i++;
    if (i == used.size()) return;
    const size_t bytes = used[i].second, off = bytes ? (size_t)((uint8_t*)p - base.p) : 0;
    used.erase(used.begin() + (long)i);
    if (!bytes) { (void)hipFree(p); return; }
    size_t k = 0;
    while (k < free_.size() && free_[k].first < off) k++;
    free_.insert(free_.begin() + (long)k, {off, bytes});
    if (k + 1 < free_.size() && free_[k].first + free_[k].second == free_[k + 1].first) { free_[k].second += free_[k + 1].second; free_.erase(free_.begin() + (long)k + 1); }
    if (k > 0 && free_[k - 1].first + free_[k - 1].second == free_[k].first) { free_[k - 1].second += free_[k].second; free_.erase(free_.begin() + (long)k); }
  }
  void release() { for (auto& u : used) if (!u.second) (void)hipFree(u.first); used.clear(); free_.clear(); base.reset(); cap = 0; }
  ~DecArena() { release(); }
};

struct DecShare {
  int device = 0, rc = 0;
  Stream s;
  std::vector<DevBuf> bufs;          // device scratch of the share, given back at release() (or early, by drop())
  // a streaming decoder's step: scratch from the decoder's own arena instead of the pool, and rows only for the first row_limit
  // block candidates at or after bit row_from.  Candidates in front of row_from are dropped, as is everything from the first
  // block candidate past the limit on: cut_bit is that candidate's bit (none: ~0).
  DecArena* arena = nullptr; std::vector<void*> abufs;
  uint32_t row_limit = ~0u; uint64_t row_from = 0, cut_bit = ~0ull;
  uint32_t ncand_seen = 0;            // candidates the magic scan found (before the row limit dropped any)
  uint64_t lo = 0, hi = 0;            // candidates starting in bytes [lo, hi) are this share's
  uint64_t up_lo = 0, up_hi = 0;      // uploaded byte range
  const uint8_t* d_in = nullptr;      // addressed by absolute byte: d_in[b] is valid for up_lo <= b < up_hi
  std::vector<Cand> cands;            // sorted by bit
  std::vector<BlockOut> bos;
  uint8_t* d_tt = nullptr;            // decoded BWT bytes of a one-batch share, tt_stride per row (several batches: packed segments)
  std::vector<uint64_t> tt_ptr;       // per candidate: device address of its decoded bytes
  // chain part
  size_t c0 = 0, c1 = 0;              // chain blocks [c0, c1) were decoded here
  uint8_t* d_w = nullptr;             // pre-RLE1 bytes of those blocks, contiguous in chain order
  RleCarry* d_carry = nullptr; uint32_t carry_tiles = 0;      // per chain block and UR_TILE-byte tile: the RLE1 expansion state at the tile start
  std::vector<uint64_t> ebase;        // element offset of block c0+i inside d_w (size c1-c0+1)
  double ms_a = 0, ms_b = 0, ms_c = 0;
  uint64_t h2d = 0, d2h = 0;          // bytes of the share's host <-> device copies
  char detail[96] = {0};            // error detail found by this share's worker thread (the detail text is per calling thread)
  // batch (cjs_bzip2_decompress_batch): input k is bytes [bst[k], ben[k]) of the upload, its blocks at most bdsz[k] bytes
  std::vector<uint32_t> bst, ben, bdsz;
  uint32_t a_batches = 0, b_batches = 0;      // row batches of phase A, inverse-BWT batches of phase B
  int take(void** p, size_t bytes) {
    if (arena) { if (!(*p = arena->take(bytes))) return (int)CJS_E_OUT_OF_MEMORY; abufs.push_back(*p); return 0; }
    DevBuf b(bytes); if (!(*p = b.p)) return (int)CJS_E_OUT_OF_MEMORY; bufs.push_back(std::move(b)); return 0;
  }
  void drop(void* p) {
    if (arena) { for (size_t i = 0; i < abufs.size(); i++) if (abufs[i] == p) { abufs.erase(abufs.begin() + (long)i); arena->give(p); return; } return; }
    for (size_t i = 0; i < bufs.size(); i++) if (bufs[i].p == p) { bufs.erase(bufs.begin() + (long)i); return; }
  }
  void release() {                    // on the share's device, once its stream has drained; again: nothing
    if (hipSetDevice(device) != hipSuccess) return;
    if (s) (void)hipStreamSynchronize(s);
    if (arena) for (void* p : abufs) arena->give(p);
    abufs.clear();
    bufs.clear();
    s.reset();
  }
  void release_keep_stream(Stream& to) { Stream keep = std::move(s); if (keep && hipSetDevice(device) == hipSuccess) (void)hipStreamSynchronize(keep); release(); to = std::move(keep); }
  uint32_t nrows_given() const { uint32_t r = 0; for (auto& c : cands) r += c.kind == 0; return r; }
  ~DecShare() { release(); }
};

// Scratch a phase takes from its share for its own duration.  done() gives all of it back, and is called only where the share's
// stream has been synchronised behind the last kernel that used it (another thread may get the memory at once).  On an error exit
// nothing goes back: the buffers stay with the share until DecShare::release(), which synchronises first.  So no destructor.
struct ShareScratch {
  DecShare* S; std::vector<void*> got;
  explicit ShareScratch(DecShare* s) : S(s) {}
  int take(void** p, size_t bytes) { const int rc = S->take(p, bytes); if (!rc) got.push_back(*p); return rc; }
  void drop(void* p) { got.erase(std::find(got.begin(), got.end(), p)); S->drop(p); }      // one buffer, early
  void done() { for (void* p : got) S->drop(p); got.clear(); }
};

struct DecJob {
  const uint8_t* in = nullptr; size_t n = 0;
  uint32_t tt_stride = 0;             // = dbuf size of the largest level in the input
  int mode = 0;
  std::vector<IbBlock> chain;         // all valid blocks in stream order (cand = index local to the decoding share)
  std::vector<uint64_t> chain_bits;
  std::vector<uint64_t> out_off;      // size chain.size()+1
  uint8_t* host = nullptr;            // final output (mode 0 / 2)
  bool timing = false;
  bool batch = false;                 // phase C: a CRC verdict for every block (crc_got) instead of stopping at the first bad one
  std::vector<uint32_t> crc_got;
  // device-resident source and sink (cjs_bzip2_decompress_device[_batch]).  upload: fills the share's scratch [0, up_hi - up_lo)
  // on its stream in place of phase A's H2D of `in`; eos: called once phase A's candidates are sorted (a batch candidate's pad
  // still names its input); dev_out: phase C expands straight into dev_out at the final offsets instead of scratch + D2H
  std::function<int(DecShare* S, uint8_t* dst)> upload;
  std::function<int(DecShare* S)> eos;
  uint8_t* dev_out = nullptr;
  // range reads: the share comes with its candidates (S->cands, sorted, kind 0) and phase A launches no magic scan.  vet, if
  // set, is called once the upload is enqueued and may erase candidates (those whose magic is not there)
  bool given = false;
  std::function<int(DecShare* S)> vet;
};

// A HIP call inside a phase: any failure is CJS_E_HIP, without a word (the phases' contract; not CJS_HIP_TRY, which prints and
// tells out-of-memory apart)
#define DEC_HIP(expr) do { if ((expr) != hipSuccess) return (int)CJS_E_HIP; } while (0)

// ---- the phases.  dec_phase_x(J, S) sets the share's device and stream, runs its steps, leaves their code in S->rc and the time in ms_x
void dec_phase_a(DecJob* J, DecShare* S);      // dec_blocks.hip: upload, magic scan, speculative decode of every candidate of the share
void dec_phase_b(DecJob* J, DecShare* S);      // dec_ibwt.hip: inverse BWT + RLE1 length pass of chain blocks [S->c0, S->c1), in batches
void dec_phase_c(DecJob* J, DecShare* S);      // dec_unrle1.hip: RLE1 expansion to the final offsets, block CRCs, D2H
size_t dec_next_batch(const DecJob* J, size_t b0, size_t c1);      // dec_ibwt.hip: the inverse-BWT batch [b0, return) of chain blocks [b0, c1)
// dec_unrle1.hip, for phase B: the RLE1 length pass over the walk's output d_w of nb blocks -> every tile's RleCarry, every block's out_len
void launch_unrle1_lengths(hipStream_t s, const uint8_t* d_w, IbBlock* d_blocks, uint32_t nb, RleCarry* d_carry, uint32_t carry_tiles);
void bad_crc_detail(char* d, size_t cap, uint32_t got, uint32_t expected);
// ---- decode.hip
double ms_since(std::chrono::steady_clock::time_point a);
int bz_header_check(const uint8_t* h, size_t n, int* level, const char** why);
int bz_max_level(const uint8_t* in, size_t n, int level, bool multistream);
int bz_block_verdict(const BlockOut& bo, uint32_t dbuf_size, uint64_t bitpos, bool timing);
uint64_t chain_out_offsets(DecJob& J);
int bunzip_core(const uint8_t* in, size_t n, int multistream, int mode, uint64_t at_bit, uint8_t** out, size_t* out_n, uint64_t* tab_pos, uint32_t* tab_size,
                long tab_cap, long* tab_n, const cjs_opts* opts, std::vector<cjs_bz_index_entry>* tab_ix = nullptr);
// ---- dec_batch.hip
struct BatchGroup;
size_t dec_group_bytes();
size_t dec_group_end(const size_t* n, size_t count, size_t k0, size_t G);
void group_verdicts(const DecJob& J, const BatchGroup& G, size_t base, size_t* off, size_t* len, int32_t* status, std::vector<std::string>& detail);
bool on_device(const void* p, int dev);        // p is memory of GPU `dev`

template <typename F>
int for_each_share(std::vector<DecShare>& sh, DecJob* J, F fn) {
  // an exception of a phase becomes the share's return code
  if (sh.size() == 1) guarded(sh[0].rc, [&] { fn(J, &sh[0]); });
  else { Workers workers; for (auto& x : sh) workers.run(x.rc, [fn, J, &x] { fn(J, &x); }); }      // (joined here)
  for (auto& x : sh) if (x.rc) { if (x.detail[0]) set_detail("%s", x.detail); return x.rc; }
  return 0;
}

// bytes a block can span: 20 bits per symbol + tables (the overlap of two shares; a streaming decoder's window behind a chunk)
constexpr uint64_t dec_extent(uint32_t tt_stride) { return (uint64_t)tt_stride * 5 / 2 + 65536; }

// Phase B's return code as a call that runs it share by share reports it.  (Phase B's own CJS_E_UNSUPPORTED / CJS_E_DATA_ERROR exits
// cannot happen -- a block holds <= 900000 bytes, a walk makes a step; should one, it is a failure of the call, reported as one of
// the call's codes.)
inline int dec_phase_b_rc(int rc) { return !rc || rc == CJS_E_OUT_OF_MEMORY || rc == CJS_E_NO_DEVICE ? rc : (int)CJS_E_HIP; }

// The chain walk of one input (Bunzip.decode :1776-1794): 32 -> end(block 0) -> end(block 1) ... over the candidates, stream CRC
// fold, multistream restarts (each member keeps its own level, :1787-1792).  in / n: the input's own bytes, whose header
// _start_bunzip has passed; positions are bits of the input.  `in` is anything indexable by byte: the host bytes, or (device
// source) an accessor over the few bytes the walk reads -- the header, and at an end-of-stream candidate the stored stream CRC and
// the restart header behind it.  at(pos, &kind, &bo) finds the candidate whose magic starts at bit
// pos (false: none) with its decode result, end_bit in bits of the input; take(bo, pos) appends a good block to the chain.
// Returns 0 or the first error the walk meets, its detail set.  mode 1 (Bunzip.table) does not test the stream CRC.
//
// `st` (a streaming decoder's step; nullptr: a walk of the whole input from its header on) holds the state the walk starts from
// and is left with the state it stopped in.  With st->partial the n bytes are only the stream so far, and the walk stops
// (st->stop != WALK_RUNS, return 0) in front of anything whose verdict the bytes still to come could change; with a row limit
// (st->cut_bit) it stops at the first candidate that was not decoded.  The state is that of the point where the walk stands:
// a later call with more bytes goes on from it.  take() sees *st as it was in front of the block it is given.
enum { WALK_RUNS = 0, WALK_ENDED, WALK_NEED_MAGIC, WALK_NEED_CRC, WALK_NEED_HEADER, WALK_NO_ROW, WALK_BLOCK_OPEN, WALK_ERR_NEAR_END, WALK_OUT_BUDGET };
struct WalkState {
  uint64_t pos = 32; uint32_t crc = 0, dbuf_size = 0;            // dbuf_size 0: from the input's header byte
  bool partial = false;
  uint64_t cut_bit = ~0ull, extent = 0;                          // extent: bytes a block can span (partial)
  int stop = WALK_RUNS;
};
template <typename Bytes, typename At, typename Take>
int bz_walk(const Bytes& in, size_t n, int multistream, int mode, uint32_t tt_stride, bool timing, At at, Take take, WalkState* st = nullptr) {
  auto read_bits = [&](uint64_t bit, int k) -> uint64_t { uint64_t v = 0; for (int i = 0; i < k; i++) { const uint64_t b = bit + i; v = (v << 1) | ((b >> 3) < n ? (in[b >> 3] >> (7 - (b & 7))) & 1u : 0u); } return v; };
  WalkState whole;
  if (!st) st = &whole;
  const bool partial = st->partial;
  uint32_t& dbuf_size = st->dbuf_size;                            // of the member stream being walked
  if (!dbuf_size) dbuf_size = 100000u * (uint32_t)(in[3] - '0');
  uint64_t& pos = st->pos; uint32_t& stream_crc = st->crc;
  auto stop = [&](int why) { st->stop = why; return 0; };
  for (;;) {
    if (partial ? pos + 48 > (uint64_t)n * 8 : (pos + 7) / 8 >= n) return stop(partial ? WALK_NEED_MAGIC : WALK_ENDED);      // inputStream.eof() (:1777)
    if (pos >= st->cut_bit) return stop(WALK_NO_ROW);
    uint32_t kind = 0; BlockOut bo;
    if (!at(pos, &kind, &bo)) return CJS_E_NOT_BZIP_DATA;        // h !== WHOLEPI (:1438)
    if (kind == 0) {
      const int rc = bz_block_verdict(bo, dbuf_size, pos, timing);
      // (partial) an error found less than a block's extent before the end may come from the zeros read past it; a good block
      // read nothing behind its end-of-block code, unless that was cut off (end_bit is clamped to the end)
      if (partial && rc && (pos >> 3) + st->extent > n) { clear_detail(); return stop(WALK_ERR_NEAR_END); }
      if (rc) return rc;
      if (partial && bo.end_bit >= (uint64_t)n * 8) return stop(WALK_BLOCK_OPEN);
      take(bo, pos);
      stream_crc = crc_fold(stream_crc, bo.crc);
      pos = bo.end_bit;
    } else {
      if (partial && (pos + 80 > (uint64_t)n * 8 || (multistream && (pos + 80 + 7) / 8 + 4 > n))) return stop(pos + 80 > (uint64_t)n * 8 ? WALK_NEED_CRC : WALK_NEED_HEADER);
      const uint32_t target = (uint32_t)read_bits(pos + 48, 32);
      pos += 80;
      if ((pos + 7) / 8 > n) pos = (uint64_t)n * 8;
      if (timing) fprintf(stderr, "[cjs dec] end of stream at bit %llu: stream crc %08x stored %08x\n", (unsigned long long)pos - 80, stream_crc, target);
      if (mode == 0 && target != stream_crc) {                   // Bunzip.table ignores the stream crc (:1852)
        set_detail("Bad stream CRC (got %x expected %x)", stream_crc, target);
        return CJS_E_DATA_ERROR;
      }
      const uint64_t byte = (pos + 7) / 8;
      if (!multistream || byte >= n) return stop(WALK_ENDED);
      // _start_bunzip again, byte aligned (:1787-1792)
      uint8_t h[4] = {0, 0, 0, 0};
      for (uint64_t i = 0; i < 4 && byte + i < n; i++) h[i] = in[byte + i];
      int lv = 0; const char* why = nullptr;
      if (bz_header_check(h, (size_t)(n - byte), &lv, &why)) { set_detail("%s", why); return CJS_E_NOT_BZIP_DATA; }
      dbuf_size = 100000u * (uint32_t)lv;
      if (dbuf_size > tt_stride) return CJS_E_UNSUPPORTED;      // cannot happen: the pre-scan saw this header
      pos = (byte + 4) * 8; stream_crc = 0;
    }
  }
}

// The candidates a walk runs over: the sorted bits of one share's candidates, or of all the shares of a single-stream call in
// share order (their byte ranges ascend), each with its share and its index there.  base: the bit of the upload at which the
// input being walked starts (a batch group: 8 x bst[i]), so that find() takes the walk's own positions.
struct WalkCands {
  const DecShare* sh;
  std::vector<uint64_t> bit; std::vector<uint32_t> share, local;
  uint64_t base = 0;
  WalkCands(const DecShare* shares, size_t nsh) : sh(shares) {
    for (size_t i = 0; i < nsh; i++)
      for (size_t k = 0; k < sh[i].cands.size(); k++) { bit.push_back(sh[i].cands[k].bit); share.push_back((uint32_t)i); local.push_back((uint32_t)k); }
  }
  long find(uint64_t pos) const {
    const auto it = std::lower_bound(bit.begin(), bit.end(), base + pos);
    return (it != bit.end() && *it == base + pos) ? (long)(it - bit.begin()) : -1;
  }
  uint32_t kind(long ci) const { return sh[share[(size_t)ci]].cands[local[(size_t)ci]].kind; }
  const BlockOut& bo(long ci) const { return sh[share[(size_t)ci]].bos[local[(size_t)ci]]; }
  IbBlock chain_block(long ci) const { return ib_block(bo(ci), sh[share[(size_t)ci]].tt_ptr[local[(size_t)ci]]); }
};

// bz_walk over C, the good blocks appended to J.chain.  met(ci, pos) is called for every candidate the walk accepts: an
// end-of-stream candidate when the walk finds it, before it reads the record behind the magic; a block once it is on the chain
// (a resumed walk's *st is then still the state in front of the block).
template <typename Bytes, typename Met>
int walk_chain(DecJob& J, const WalkCands& C, const Bytes& in, size_t n, int multistream, int mode, Met met, WalkState* st = nullptr) {
  long last = -1;
  return bz_walk(in, n, multistream, mode, J.tt_stride, J.timing,
                 [&](uint64_t pos, uint32_t* kind, BlockOut* bo) {
                   if ((last = C.find(pos)) < 0) return false;
                   *kind = C.kind(last); *bo = C.bo(last); bo->end_bit -= C.base;
                   if (*kind) met(last, pos);
                   return true;
                 },
                 [&](const BlockOut&, uint64_t pos) { J.chain.push_back(C.chain_block(last)); met(last, pos); }, st);
}
inline void met_nothing(long, uint64_t) {}

// One share after phase A whose chain (J.chain) the caller has picked itself -- recovery: every decodable candidate; range reads:
// the blocks that agree with their index entries -- with J.batch set: phases B and C over one inverse-BWT batch [g0, g1) of it at a
// time (dec_next_batch), phase C expanding into scratch d_exp of the batch's size with J.out_off local to the batch and a CRC
// verdict per block (J.crc_got).  use(g0, g1, d_exp, q) is the caller's selection and copies; it returns with the stream drained,
// and what it took through q goes back behind the batch's own three buffers.  Phase B gives a one-batch share's rows back when it
// ends; here it runs once per batch, so the rows are kept to the end.  The memory held is phase A's plus one batch's, however many
// blocks there are.  0, or a failure of the call (nothing goes back then: the share's release() does it).
template <typename Use>
int dec_scratch_batches(DecJob& J, DecShare& S, Use use) {
  uint8_t* rows = S.d_tt; S.d_tt = nullptr;
  const size_t nb = J.chain.size();
  J.crc_got.assign(nb, 0);
  J.out_off.assign(nb + 1, 0);
  for (size_t g0 = 0; g0 < nb;) {
    const size_t g1 = dec_next_batch(&J, g0, nb);
    S.c0 = g0; S.c1 = g1; S.rc = 0;
    guarded(S.rc, [&] { dec_phase_b(&J, &S); });
    if (S.rc) return dec_phase_b_rc(S.rc);
    J.out_off[g0] = 0;                                            // (offsets inside the batch's scratch)
    for (size_t k = g0; k < g1; k++) J.out_off[k + 1] = J.out_off[k] + J.chain[k].out_len;
    uint8_t* d_exp = nullptr;
    CJS_TRY(S.take((void**)&d_exp, (size_t)J.out_off[g1] + 64));
    J.dev_out = d_exp; J.host = nullptr;
    guarded(S.rc, [&] { dec_phase_c(&J, &S); });
    if (S.rc) return S.rc;
    ShareScratch q(&S);
    CJS_TRY(use(g0, g1, d_exp, q));
    S.drop(d_exp); S.drop(S.d_w); S.drop(S.d_carry);              // (the stream has drained)
    q.done();
    S.d_w = nullptr; S.d_carry = nullptr;
    g0 = g1;
  }
  if (rows) S.drop(rows);
  return 0;
}

// ---- a batch group (host form: dec_batch_group, device form: dev_group_*; dec_batch.hip)
struct BatchGroup {
  size_t k0 = 0, k1 = 0;              // inputs [k0, k1) of the call
  std::vector<uint8_t> ok;            // input k0 + i passed _start_bunzip
  std::vector<size_t> ch0, ch1;       // input k0 + i's chain blocks
};

// The layout of a group: _start_bunzip (:1408-1427) of every input, the accepted ones at 4-byte-aligned offsets of one upload
// (S.bst / S.ben), each with the block size of its own single call (S.bdsz: the kernels' limits for its blocks), the rows sized
// for the largest of them.  hdr(k): the first bytes of input k; level(k, lv): its largest member level, lv being its header's;
// placed(k, at): input k lies at byte `at` of the upload.
template <typename Hdr, typename Level, typename Placed>
void group_layout(DecJob& J, DecShare& S, BatchGroup& G, size_t k0, size_t k1, const size_t* n, int32_t* status, std::vector<std::string>& detail,
                  Hdr hdr, Level level, Placed placed) {
  const size_t items = k1 - k0;
  G.k0 = k0; G.k1 = k1; G.ok.assign(items, 0);
  J.mode = 0; J.batch = true; J.timing = env_debug();
  S.bst.resize(items); S.ben.resize(items); S.bdsz.assign(items, 100000u);
  int max_level = 1;
  size_t bytes = 0;
  for (size_t i = 0; i < items; i++) {
    const size_t k = k0 + i;
    S.bst[i] = S.ben[i] = (uint32_t)bytes;
    int lv = 0; const char* why = nullptr;
    if ((status[k] = bz_header_check(hdr(k), n[k], &lv, &why)) != 0) { detail[k] = why; continue; }
    const int own = level(k, lv);
    S.bdsz[i] = 100000u * (uint32_t)own;
    max_level = std::max(max_level, own);
    G.ok[i] = 1;
    placed(k, bytes);
    S.ben[i] = (uint32_t)(bytes + n[k]);
    bytes = (bytes + n[k] + 3) & ~(size_t)3;
  }
  J.tt_stride = 100000u * (uint32_t)max_level;
  J.n = bytes;
  S.lo = 0; S.hi = bytes; S.up_lo = 0; S.up_hi = bytes;
}

// A laid-out group up to phase B: phase A over the upload, the walk of every accepted input over the candidates of its bytes
// (walk(k, C), C.base being the input's first bit of the upload; its error is pending: a bad block CRC in front of it wins),
// phase B over all chain blocks, the output offsets.  A failure of the call, or 0 and the bytes of the group's output.
template <typename Walk>
int group_prepare(DecJob& J, DecShare& S, BatchGroup& G, int32_t* status, std::vector<std::string>& detail, Walk walk, uint64_t* total) {
  if (J.n) {
    guarded(S.rc, [&] { dec_phase_a(&J, &S); });
    if (S.rc) return S.rc;
  }
  WalkCands C(&S, 1);
  const size_t items = G.k1 - G.k0;
  G.ch0.assign(items, 0); G.ch1.assign(items, 0);
  for (size_t i = 0; i < items; i++) {
    G.ch0[i] = G.ch1[i] = J.chain.size();
    if (!G.ok[i]) continue;
    C.base = 8ull * S.bst[i];
    clear_detail();
    const int rc = walk(G.k0 + i, C);
    G.ch1[i] = J.chain.size();
    if (rc) { status[G.k0 + i] = rc; detail[G.k0 + i] = cjs_last_error_detail(); }
  }
  clear_detail();
  S.c0 = 0; S.c1 = J.chain.size();
  if (S.c1) {
    guarded(S.rc, [&] { dec_phase_b(&J, &S); });
    if (S.rc) return dec_phase_b_rc(S.rc);
  }
  *total = chain_out_offsets(J);
  return 0;
}

}  // namespace cjs
