// linekeys.hip -- a key per line of an indexed .bz2 stream (cjs_bzip2_line_keys[_device]): the sixth consumer of the
// pass engine of the indexed entry points (range_engine.h).  Every decoded inverse-BWT batch is hashed where it stands expanded
// in device scratch; 16 bytes per newline and 32 per block leave the GPU.
//   lk_summary  per 16 KiB tile of a block: the number of newlines in it, the fragment behind its last newline
//   lk_chain    per block: the exclusive scan of its tile counts and its total; the tiles' fragments chained into every tile's
//               carry-in (the fragment between the block's last newline in front of the tile and the tile); the block's tail
//   lk_emit     per tile again: a record per newline at rank = the tile's scanned count + the rank in the tile
// cjs_bzip2_tally[_device] runs the same passes with a second destination: the records stay in a device array of the
// window's lines (lk_heads brings down a block's first record alone, lk_patch puts the joined ones up) and tally.hip groups them.
// The arithmetic of the key and of the join is line_key.h; the line diff over the keys is line_diff.h (both without HIP).
// Tile geometry is that of lines.hip (ln_count / ln_scan, restated here with the hash beside the count): a tile never spans two
// blocks.  A thread takes a contiguous share of its tile's 16-byte vectors (4 or 5 of them) and walks it byte by byte, two
// Horner steps a byte; the shares are joined by a segmented scan (a share with a newline cuts what stands in front of it off).
#include "range_engine.h"
#include "bz_lines.h"
#include "line_key.h"
#include "line_diff.h"
#include "tally.h"
#include "sort.h"
#include "cut_plan.h"
#include <algorithm>
#include <string.h>

using namespace cjs;

namespace cjs {

constexpr uint32_t LK_TILE = 16384;                        // bytes of a tile: that of the line table
struct LkBlk { uint64_t src, rec0; uint32_t len, tile0, nrec, blk; };      // len bytes at src; its records from rec0 on, nrec of them by the table
struct LkOpen { uint64_t h1, h2; uint32_t len, has; };                     // a tile's open fragment (lk_summary), then its carry-in (lk_chain)
struct LkTail { uint64_t h1, h2, head_h2; uint32_t len, pad; };            // per block: the fragment behind its last newline; H_B2 of its first record in full

__host__ __device__ __forceinline__ uint32_t lk_tiles(uint32_t len) { return (len + LK_TILE - 1) / LK_TILE; }

// An element of the segmented scan: a fragment with the powers of its length, and whether a newline stands in front of it.
struct LkEl { uint64_t h1, h2, p1, p2; uint32_t len, has; };
__device__ __forceinline__ LkEl lk_none() { return LkEl{0, 0, 1, 1, 0, 0}; }
__device__ __forceinline__ LkEl lk_comb(const LkEl& a, const LkEl& b) {      // a, then b
  if (b.has) return b;
  return LkEl{lk_add(lk_mul(a.h1, b.p1), b.h1), lk_add(lk_mul(a.h2, b.p2), b.h2), lk_mul(a.p1, b.p1), lk_mul(a.p2, b.p2), a.len + b.len, a.has};
}
__device__ __forceinline__ LkEl lk_el(const LkBases& B, uint64_t h1, uint64_t h2, uint32_t len, uint32_t has) {
  return LkEl{h1, h2, lk_pow(B.b1, len), lk_pow(B.b2, len), len, has};
}
__device__ __forceinline__ LkEl lk_shfl_up(const LkEl& e, int d) {
  return LkEl{__shfl_up(e.h1, d, 64), __shfl_up(e.h2, d, 64), __shfl_up(e.p1, d, 64), __shfl_up(e.p2, d, 64), __shfl_up(e.len, d, 64), __shfl_up(e.has, d, 64)};
}
// Workgroup of 256: the combination of the elements in front of this thread's, `total` = of all of them.  sm: four elements.
// (How the six shuffles a step and the four elements of LDS sit on the banks is not measured.)
__device__ __forceinline__ LkEl lk_block_excl(const LkEl& v, LkEl* sm, LkEl& total) {
  LkEl x = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const LkEl y = lk_shfl_up(x, d);
    if (lane_id() >= d) x = lk_comb(y, x);
  }
  if (lane_id() == 63) sm[wave_id()] = x;
  LkEl prev = lk_shfl_up(x, 1);
  if (lane_id() == 0) prev = lk_none();
  __syncthreads();
  LkEl base = lk_none();
  total = lk_none();
  for (int w = 0; w < 4; w++) {
    if (w == wave_id()) base = total;
    total = lk_comb(total, sm[w]);
  }
  __syncthreads();
  return lk_comb(base, prev);
}

// f(byte) for every byte of the tile in vectors [v0, v1) of its span, in order (a vector's bytes outside the tile are left out)
template <typename F>
__device__ __forceinline__ void lk_bytes(const RgSpan& S, uint32_t v0, uint32_t v1, F f) {
  const uint64_t end = S.a0 + S.n;
  for (uint32_t v = v0; v < v1; v++) {
    const uint64_t a = S.base + 16ull * v;
    const uint4 x = rg_vec(S, v);
    const uint32_t w[4] = {x.x, x.y, x.z, x.w};
    const uint32_t lo = a < S.a0 ? (uint32_t)(S.a0 - a) : 0u, hi = end - a < 16 ? (uint32_t)(end - a) : 16u;
#pragma unroll
    for (uint32_t i = 0; i < 16; i++) if (i >= lo && i < hi) f((uint8_t)(w[i >> 2] >> (8 * (i & 3))));
  }
}

struct LkTileOf { LkBlk g; RgSpan S; uint32_t v0, v1; };
// tile t: its block, its span, this thread's share of the span's vectors
__device__ __forceinline__ LkTileOf lk_tile_of(const LkBlk* __restrict__ blks, uint32_t nblk, uint32_t t) {
  LkTileOf T;
  T.g = rg_seg_of(blks, nblk, t);
  const uint32_t p0 = (t - T.g.tile0) * LK_TILE;
  T.S = rg_span(T.g.src + p0, min(LK_TILE, T.g.len - p0));
  const uint32_t per = (T.S.nvec + 255) / 256;
  T.v0 = min(threadIdx.x * per, T.S.nvec); T.v1 = min(T.v0 + per, T.S.nvec);
  return T;
}

__global__ __launch_bounds__(256) void lk_summary(const LkBlk* __restrict__ blks, uint32_t nblk, LkBases B, uint32_t* __restrict__ cnt, LkOpen* __restrict__ open) {
  __shared__ LkEl sm[4];
  __shared__ uint32_t sc[4];
  const LkTileOf T = lk_tile_of(blks, nblk, blockIdx.x);
  LkFrag f{0, 0, 0};
  uint32_t c = 0;
  lk_bytes(T.S, T.v0, T.v1, [&](uint8_t ch) {
    lk_push(f, B, ch);
    if (ch == 0x0A) { c++; f = LkFrag{0, 0, 0}; }
  });
  LkEl total;
  lk_block_excl(lk_el(B, f.h1, f.h2, (uint32_t)f.len, c ? 1u : 0u), sm, total);
  const uint32_t n = block_sum<256, uint32_t>(c, sc);
  if (threadIdx.x == 0) { cnt[blockIdx.x] = n; open[blockIdx.x] = LkOpen{total.h1, total.h2, total.len, total.has}; }
}

// block blockIdx.x: the counts of its tiles -> their exclusive prefix sums, tot = their sum; the open fragments of its tiles -> the
// fragment that stands open in front of each; tail = the one behind the last
__global__ __launch_bounds__(256) void lk_chain(const LkBlk* __restrict__ blks, LkBases B, uint32_t* __restrict__ cnt, LkOpen* __restrict__ open,
                                                uint32_t* __restrict__ tot, LkTail* __restrict__ tail) {
  __shared__ LkEl sm[4];
  __shared__ uint32_t sc[4];
  const LkBlk g = blks[blockIdx.x];
  const uint32_t nt = lk_tiles(g.len);
  uint32_t* c = cnt + g.tile0;
  LkOpen* o = open + g.tile0;
  uint32_t run = 0;
  LkEl carry = lk_none();
  for (uint32_t b = 0; b < nt; b += 256) {
    const uint32_t i = b + threadIdx.x, v = i < nt ? c[i] : 0;
    LkEl e = lk_none();
    if (i < nt) { const LkOpen x = o[i]; e = lk_el(B, x.h1, x.h2, x.len, x.has); }
    uint32_t sum;
    const uint32_t ex = block_excl_sum<256, uint32_t>(v, sc, sum);
    LkEl total;
    const LkEl in = lk_comb(carry, lk_block_excl(e, sm, total));
    if (i < nt) { c[i] = run + ex; o[i] = LkOpen{in.h1, in.h2, in.len, in.has}; }
    run += sum;
    carry = lk_comb(carry, total);
  }
  if (threadIdx.x == 0) { tot[blockIdx.x] = run; tail[blockIdx.x] = LkTail{carry.h1, carry.h2, 0, carry.len, 0}; }
}

// Newline number r of the block (from 0; ranks ascend with the tile, the thread and the byte) -> out[rec0 + r]: the key of the
// fragment from the newline in front of it, or from the block's first byte, up to and including it.  No atomics: the ranks come
// from the scanned tile counts and the workgroup's prefix sums.  Launched only when every block's total is its nrec.
__global__ __launch_bounds__(256) void lk_emit(const LkBlk* __restrict__ blks, uint32_t nblk, LkBases B, const uint32_t* __restrict__ cnt,
                                               const LkOpen* __restrict__ open, cjs_bz_linekey* __restrict__ out, LkTail* __restrict__ tail) {
  __shared__ LkEl sm[4];
  __shared__ uint32_t sc[4];
  const LkTileOf T = lk_tile_of(blks, nblk, blockIdx.x);
  uint32_t c = 0;
  for (uint32_t v = T.v0; v < T.v1; v++) c += ln_count16(rg_vec(T.S, v));      // (bytes outside the tile read as zeros)
  uint32_t in_tile;
  const uint32_t ex = block_excl_sum<256, uint32_t>(c, sc, in_tile);
  if (!in_tile) return;                                                       // a tile without a newline writes nothing
  const uint32_t r0 = cnt[blockIdx.x] + ex;                                   // the rank in the block of this thread's first newline
  cjs_bz_linekey* mine = out + T.g.rec0 + r0;
  LkFrag f{0, 0, 0}, head{0, 0, 0};
  uint32_t j = 0;
  lk_bytes(T.S, T.v0, T.v1, [&](uint8_t ch) {
    lk_push(f, B, ch);
    if (ch != 0x0A) return;
    if (j == 0) head = f;
    else if (r0 + j < T.g.nrec) mine[j] = lk_key(f);
    j++; f = LkFrag{0, 0, 0};
  });
  LkEl total;
  const LkEl shares = lk_block_excl(lk_el(B, f.h1, f.h2, (uint32_t)f.len, j ? 1u : 0u), sm, total);
  if (!j || r0 >= T.g.nrec) return;
  const LkOpen x = open[blockIdx.x];                                          // what stands open in front of the tile ...
  const LkEl in = lk_comb(LkEl{x.h1, x.h2, 1, 1, x.len, x.has}, shares);      // ... and in front of this share
  const LkFrag first = lk_join_pw(LkFrag{in.h1, in.h2, in.len}, head, lk_pow(B.b1, head.len), lk_pow(B.b2, head.len));
  mine[0] = lk_key(first);
  if (r0 == 0) tail[T.g.blk].head_h2 = first.h2;
}

// The tally keeps the records on the device; the host join needs the first one of every block: head[i] = block i's, if it has one.
__global__ __launch_bounds__(256) void lk_heads(const LkBlk* __restrict__ blks, uint32_t nblk, const cjs_bz_linekey* __restrict__ rec, cjs_bz_linekey* __restrict__ head) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nblk) return;
  const LkBlk g = blks[i];
  head[i] = g.nrec ? rec[g.rec0] : cjs_bz_linekey{0, 0, 0};
}
// ... and the joined records of the lines that span blocks go up at the end: keys[p[i].at] = p[i].key (no `at` twice with two values)
struct LkPatch { uint64_t at; cjs_bz_linekey key; };
__global__ __launch_bounds__(256) void lk_patch(cjs_bz_linekey* __restrict__ keys, const LkPatch* __restrict__ p, uint32_t np) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < np) keys[p[i].at] = p[i].key;
}

}  // namespace cjs

// ---------------------------------------------------------------- the driver
namespace {

bool lines_belong(const cjs_bz_index* ix, const cjs_bz_lines* t) {
  if (t->nl.size() == ix->e.size() && t->total_bytes == ix->off.back() && t->crc_fold == bz_lines_fold(ix)) return true;
  set_detail("the line table is of another index");
  return false;
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

// The touched blocks of the window [first, end) of lines: from the block of newline number `first` through the block of newline
// number `end`, the line table's routing of a line's start
std::vector<uint32_t> window_blocks(const cjs_bz_index* idx, const cjs_bz_lines* t, uint64_t first, uint64_t end) {
  std::vector<uint32_t> touched;
  if (idx->e.empty()) return touched;
  const uint64_t N = t->cum.back();
  const LineRoute r0 = route_locate(t->cum, t->total_bytes, first), r1 = route_locate(t->cum, t->total_bytes, end);
  const size_t b0 = first ? r0.block : 0, b1 = end <= N ? r1.block : idx->e.size() - 1;
  for (size_t b = b0; b <= b1; b++) if (idx->e[b].size) touched.push_back((uint32_t)b);
  return touched;
}

struct LineKeysCall {
  const cjs_bz_index* ix = nullptr;
  const cjs_bz_lines* t = nullptr;
  LkJoin J;
  uint64_t h2d = 0, d2h = 0, tiles = 0;

  int batch(const RangeBatch& B) {
    std::vector<LkBlk> blks; std::vector<uint32_t> which;
    uint64_t nt = 0, nrec = 0;
    for (size_t k = B.g0; k < B.g1; k++) {
      const uint32_t b = B.blk[k];
      const uint32_t len = ix->e[b].size;
      if (!B.V.good(b) || !len) continue;
      blks.push_back(LkBlk{B.addr(k), nrec, len, (uint32_t)nt, t->nl[b], (uint32_t)blks.size()});
      which.push_back(b);
      nt += lk_tiles(len); nrec += t->nl[b];
    }
    if (blks.empty()) return 0;
    if (nt > 0x7FFFFFFFull) return CJS_E_UNSUPPORTED;
    const size_t nblk = blks.size();
    auto pad = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t o_blk = 0, o_cnt = o_blk + pad(sizeof(LkBlk) * nblk), o_open = o_cnt + pad(4 * (size_t)nt), o_tot = o_open + pad(sizeof(LkOpen) * (size_t)nt),
                 o_tail = o_tot + pad(4 * nblk), o_rec = o_tail + pad(sizeof(LkTail) * nblk), o_head = o_rec + pad(sizeof(cjs_bz_linekey) * (size_t)nrec),
                 bytes = o_head + (J.d_keys ? pad(sizeof(cjs_bz_linekey) * nblk) : 0);
    DevBuf mem(bytes);
    if (!mem.p) return CJS_E_OUT_OF_MEMORY;
    uint8_t* d = (uint8_t*)mem.p;
    LkBlk* d_blk = (LkBlk*)(d + o_blk); uint32_t* d_cnt = (uint32_t*)(d + o_cnt); LkOpen* d_open = (LkOpen*)(d + o_open);
    uint32_t* d_tot = (uint32_t*)(d + o_tot); LkTail* d_tail = (LkTail*)(d + o_tail); cjs_bz_linekey* d_rec = (cjs_bz_linekey*)(d + o_rec);
    cjs_bz_linekey* d_head = (cjs_bz_linekey*)(d + o_head);                             // (the tally alone)
    std::vector<uint32_t> tot(nblk); std::vector<LkTail> tails(nblk);
    // what comes down: every record, or for the tally the first one of every block (pinned from 1 MiB on: the records of 100 MB of text are 14 MB)
    const size_t down = J.d_keys ? nblk : (size_t)nrec;
    HostBuf staged(sizeof(cjs_bz_linekey) * std::max<size_t>(down, 1));
    if (!staged.p) return CJS_E_OUT_OF_MEMORY;
    cjs_bz_linekey* recs = (cjs_bz_linekey*)staged.p;
    hipStream_t s = B.s;
    int rc = 0;
    // from here on no way out without a synchronize: the copies may still be reading or writing the vectors
    if (hipMemcpyAsync(d_blk, blks.data(), sizeof(LkBlk) * nblk, hipMemcpyHostToDevice, s) != hipSuccess) rc = CJS_E_HIP;
    else {
      hipLaunchKernelGGL(lk_summary, dim3((unsigned)nt), dim3(256), 0, s, (const LkBlk*)d_blk, (uint32_t)nblk, J.B, d_cnt, d_open);
      hipLaunchKernelGGL(lk_chain, dim3((unsigned)nblk), dim3(256), 0, s, (const LkBlk*)d_blk, J.B, d_cnt, d_open, d_tot, d_tail);
      if (hipGetLastError() != hipSuccess || hipMemcpyAsync(tot.data(), d_tot, 4 * nblk, hipMemcpyDeviceToHost, s) != hipSuccess) rc = CJS_E_HIP;
    }
    CJS_TRY(drained(s, rc));
    // the records are written at the table's ranks: only over blocks that have the table's newlines
    for (size_t i = 0; i < nblk; i++)
      if (tot[i] != blks[i].nrec) { set_detail("line table does not match the stream at block %u", which[i]); return CJS_E_DATA_ERROR; }
    hipLaunchKernelGGL(lk_emit, dim3((unsigned)nt), dim3(256), 0, s, (const LkBlk*)d_blk, (uint32_t)nblk, J.B, (const uint32_t*)d_cnt, (const LkOpen*)d_open, d_rec, d_tail);
    if (J.d_keys) {
      // the records of the window go to their ranks in the device array, a copy per run of blocks whose ranks follow one another
      // (the first record of a block is not yet its line's key: the join's patch follows at the end)
      uint64_t run_dst = 0, run_src = 0, run_n = 0;
      auto flush = [&] {
        if (run_n && hipMemcpyAsync(J.d_keys + run_dst, d_rec + run_src, sizeof(cjs_bz_linekey) * (size_t)run_n, hipMemcpyDeviceToDevice, s) != hipSuccess) rc = CJS_E_HIP;
        run_n = 0;
      };
      for (size_t i = 0; i < nblk; i++) {
        const uint64_t l0 = t->cum[which[i]], lo = std::max<uint64_t>(l0, J.first), hi = std::min<uint64_t>(l0 + blks[i].nrec, J.end);
        if (lo >= hi) continue;
        if (run_n && (run_dst + run_n != lo - J.first || run_src + run_n != blks[i].rec0 + (lo - l0))) flush();
        if (!run_n) { run_dst = lo - J.first; run_src = blks[i].rec0 + (lo - l0); }
        run_n += hi - lo;
      }
      flush();
      hipLaunchKernelGGL(lk_heads, dim3((unsigned)((nblk + 255) / 256)), dim3(256), 0, s, (const LkBlk*)d_blk, (uint32_t)nblk, (const cjs_bz_linekey*)d_rec, d_head);
    }
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(tails.data(), d_tail, sizeof(LkTail) * nblk, hipMemcpyDeviceToHost, s) != hipSuccess ||
        (down && hipMemcpyAsync(recs, J.d_keys ? d_head : d_rec, sizeof(cjs_bz_linekey) * down, hipMemcpyDeviceToHost, s) != hipSuccess)) rc = CJS_E_HIP;
    CJS_TRY(drained(s, rc));
    h2d += sizeof(LkBlk) * nblk; d2h += 4 * nblk + sizeof(LkTail) * nblk + sizeof(cjs_bz_linekey) * down; tiles += nt;
    for (size_t i = 0; i < nblk; i++) J.good(which[i], recs + (J.d_keys ? i : blks[i].rec0), tails[i]);
    return 0;
  }
};

int line_keys_core(const uint8_t* in, const uint8_t* d_in, size_t n, const cjs_bz_index* idx, const cjs_bz_lines* t, uint64_t first, uint64_t count,
                   uint64_t seed, cjs_bz_linekey* keys, size_t cap, cjs_bz_linekeys_info* info, const cjs_opts* opts) {
  clear_detail();
  if (!idx || !t || !info || (!keys && cap)) return CJS_E_INVALID_ARG;
  CJS_TRY(check_index_stream(in ? in : d_in, n, idx));
  if (!lines_belong(idx, t)) return CJS_E_INVALID_ARG;
  info->n_lines = info->n_bad_blocks = info->blocks_decoded = 0; info->first_bad_block = ~0ull;
  const uint64_t N = t->cum.back();
  const uint64_t end = first + count < first ? N + 1 : std::min(first + count, N + 1);      // (the add saturates)
  if (first >= end) return 0;
  info->n_lines = end - first;
  if (!cap) return 0;                                              // the count query: the table alone
  const std::vector<uint32_t> touched = window_blocks(idx, t, first, end);
  LineKeysCall C;
  C.ix = idx; C.t = t;
  C.J.t = t; C.J.B = lk_bases(seed); C.J.first = first; C.J.end = end; C.J.keys = keys; C.J.cap = cap; C.J.touched = &touched;
  RangeStats st;
  RangeVerdicts V(idx);
  if (!touched.empty()) {
    CallDevice cd;
    CJS_TRY(cd.select(opts));
    if (d_in && !on_device(d_in, cd.dev)) return CJS_E_INVALID_ARG;      // (no host pointer reaches a kernel)
    CJS_TRY(range_engine(in, d_in, idx, touched, V, cd.dev, st, [&](const RangeBatch& B) { return C.batch(B); }));
  }
  C.J.finish();
  info->blocks_decoded = touched.size();
  const BadBlocks bad = V.bad_among(touched);
  info->n_bad_blocks = bad.n; info->first_bad_block = bad.first;
  if (bad.n) V.set_bad_detail(idx, (size_t)bad.first);
  if (env_debug())
    fprintf(stderr, "[cjs linekeys] %s: lines [%llu, %llu), %zu of %zu blocks touched, %llu bad, %u passes (%u row batches, %u inverse-BWT batches), upload %llu B, "
            "%llu tiles, H2D %llu D2H %llu\n", d_in ? "device" : "host", (unsigned long long)first, (unsigned long long)end, touched.size(), idx->e.size(),
            (unsigned long long)bad.n, st.passes, st.a_batches, st.b_batches, (unsigned long long)st.up, (unsigned long long)C.tiles,
            (unsigned long long)(st.h2d + C.h2d), (unsigned long long)(st.d2h + C.d2h));
  return 0;
}

// ---- the keys of the lines of plain text in device memory (the tally of a cut; cjs_stage_text_keys_device)
// The text is cut into pieces of at most `piece` bytes, and the kernels see a piece as they see a block: lk_summary and lk_chain
// over all pieces at once, the pieces' totals come down and set rec0 / nrec (a piece's record count is not known before), lk_emit
// writes the records at their ranks straight into d_keys, lk_heads brings the first record of every piece down, and the same LkJoin
// that joins blocks joins the pieces over a table made of those totals: a patch per piece with a newline, and the tail.
constexpr size_t LK_PIECE = 900000;
size_t text_keys_pieces(size_t n, size_t piece) { return (n + piece - 1) / piece; }
size_t text_keys_work_bytes(size_t n, size_t piece) {
  auto pad = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t np = text_keys_pieces(n, piece), nt = n / LK_TILE + np + 1;
  return pad(sizeof(LkBlk) * np) + pad(4 * nt) + pad(sizeof(LkOpen) * nt) + pad(4 * np) + pad(sizeof(LkTail) * np) + pad(sizeof(cjs_bz_linekey) * np) +
         pad(sizeof(LkPatch) * (np + 1)) + 256;
}
// d_text[0 .. n) -> d_keys (room for key_cap records), in the workspace d_work of text_keys_work_bytes(n, piece) bytes, on stream s.
// tally_tail: the tally's rule for the tail (an empty one is no line, another is keyed with a newline), else a record for the tail
// whatever it is, as cjs_stage_line_keys gives one.  *n_keys = the records written.  Returns with s drained.
int text_keys_device(hipStream_t s, const uint8_t* d_text, size_t n, const LkBases& B, size_t piece, bool tally_tail, cjs_bz_linekey* d_keys, size_t key_cap,
                     uint8_t* d_work, uint64_t* n_keys, uint64_t* h2d, uint64_t* d2h) {
  auto pad = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t np = text_keys_pieces(n, piece);
  std::vector<LkBlk> blks(np);
  uint64_t nt = 0;
  for (size_t i = 0; i < np; i++) {
    const uint32_t len = (uint32_t)std::min(piece, n - i * piece);
    blks[i] = LkBlk{(uint64_t)(uintptr_t)(d_text + i * piece), 0, len, (uint32_t)nt, 0, (uint32_t)i};
    nt += lk_tiles(len);
  }
  if (nt > 0x7FFFFFFFull || np > 0x7FFFFFFFull) return drained(s, CJS_E_UNSUPPORTED);
  const size_t o_blk = 0, o_cnt = o_blk + pad(sizeof(LkBlk) * np), o_open = o_cnt + pad(4 * (size_t)nt), o_tot = o_open + pad(sizeof(LkOpen) * (size_t)nt),
               o_tail = o_tot + pad(4 * np), o_head = o_tail + pad(sizeof(LkTail) * np), o_patch = o_head + pad(sizeof(cjs_bz_linekey) * np);
  LkBlk* d_blk = (LkBlk*)(d_work + o_blk); uint32_t* d_cnt = (uint32_t*)(d_work + o_cnt); LkOpen* d_open = (LkOpen*)(d_work + o_open);
  uint32_t* d_tot = (uint32_t*)(d_work + o_tot); LkTail* d_tail = (LkTail*)(d_work + o_tail); cjs_bz_linekey* d_head = (cjs_bz_linekey*)(d_work + o_head);
  LkPatch* d_patch = (LkPatch*)(d_work + o_patch);
  std::vector<uint32_t> tot(np); std::vector<LkTail> tails(np); std::vector<cjs_bz_linekey> heads(np);
  cjs_bz_lines table;                                       // the pieces' newlines as a line table: what LkJoin reads of one
  table.cum.assign(1, 0);
  int rc = 0;
  if (np) {
    if (hipMemcpyAsync(d_blk, blks.data(), sizeof(LkBlk) * np, hipMemcpyHostToDevice, s) != hipSuccess) rc = CJS_E_HIP;
    else {
      hipLaunchKernelGGL(lk_summary, dim3((unsigned)nt), dim3(256), 0, s, (const LkBlk*)d_blk, (uint32_t)np, B, d_cnt, d_open);
      hipLaunchKernelGGL(lk_chain, dim3((unsigned)np), dim3(256), 0, s, (const LkBlk*)d_blk, B, d_cnt, d_open, d_tot, d_tail);
      if (hipGetLastError() != hipSuccess || hipMemcpyAsync(tot.data(), d_tot, 4 * np, hipMemcpyDeviceToHost, s) != hipSuccess) rc = CJS_E_HIP;
    }
    CJS_TRY(drained(s, rc));
    for (size_t i = 0; i < np; i++) {
      blks[i].rec0 = table.cum.back(); blks[i].nrec = tot[i];
      table.nl.push_back(tot[i]); table.cum.push_back(table.cum.back() + tot[i]);
    }
  }
  const uint64_t total = table.cum.back();
  if (total >= key_cap) return CJS_E_HIP;                   // (cannot be: the caller's room is the lines of the text, and one for the tail)
  std::vector<uint32_t> all(np);
  for (size_t i = 0; i < np; i++) all[i] = (uint32_t)i;
  LkJoin J;
  J.t = &table; J.B = B; J.first = 0; J.end = total + 1; J.cap = (size_t)total + 1; J.touched = &all; J.d_keys = d_keys; J.tally_tail = tally_tail;
  if (np) {
    if (hipMemcpyAsync(d_blk, blks.data(), sizeof(LkBlk) * np, hipMemcpyHostToDevice, s) != hipSuccess) rc = CJS_E_HIP;
    else {
      hipLaunchKernelGGL(lk_emit, dim3((unsigned)nt), dim3(256), 0, s, (const LkBlk*)d_blk, (uint32_t)np, B, (const uint32_t*)d_cnt, (const LkOpen*)d_open, d_keys, d_tail);
      hipLaunchKernelGGL(lk_heads, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, s, (const LkBlk*)d_blk, (uint32_t)np, (const cjs_bz_linekey*)d_keys, d_head);
      if (hipGetLastError() != hipSuccess || hipMemcpyAsync(tails.data(), d_tail, sizeof(LkTail) * np, hipMemcpyDeviceToHost, s) != hipSuccess ||
          hipMemcpyAsync(heads.data(), d_head, sizeof(cjs_bz_linekey) * np, hipMemcpyDeviceToHost, s) != hipSuccess) rc = CJS_E_HIP;
    }
    CJS_TRY(drained(s, rc));
    for (size_t i = 0; i < np; i++) J.good((uint32_t)i, &heads[i], tails[i]);
  }
  J.finish();
  const size_t npatch = J.patches.size();
  if (npatch > np + 1) return CJS_E_HIP;
  if (npatch) {
    if (hipMemcpyAsync(d_patch, J.patches.data(), sizeof(LkPatch) * npatch, hipMemcpyHostToDevice, s) != hipSuccess) rc = CJS_E_HIP;
    else hipLaunchKernelGGL(lk_patch, dim3((unsigned)((npatch + 255) / 256)), dim3(256), 0, s, d_keys, (const LkPatch*)d_patch, (uint32_t)npatch);
    if (!rc && hipGetLastError() != hipSuccess) rc = CJS_E_HIP;
  }
  *n_keys = total + 1 - (J.tail_dropped ? 1 : 0);
  if (h2d) *h2d += 2 * sizeof(LkBlk) * np + sizeof(LkPatch) * npatch;
  if (d2h) *d2h += (4 + sizeof(LkTail) + sizeof(cjs_bz_linekey)) * np;
  return drained(s, rc);
}

// The tally of a cut (modes CJS_CUT_FIELDS / CJS_CUT_BYTES), a composition: cjs_bzip2_cut_device into a pooled buffer of the touched
// blocks' bytes + 1 (never less than the window's bytes + 1, which the cut's contract says is enough), the keys of that text's lines
// (text_keys_device), the grouping.  The host form uploads the stream first, as the passes would.  A bad block fails the call as it
// fails the cut.  Everything is sized from the tables and taken before the cut runs.
int tally_cut(const uint8_t* in, const uint8_t* d_in, size_t n, const cjs_bz_index* idx, const cjs_bz_lines* t, uint64_t first, uint64_t end, uint64_t count,
              uint64_t seed, uint32_t mode, uint32_t delim, const cjs_cut_range* sel, uint32_t nsel, uint32_t order, uint64_t min_count, uint64_t max_count,
              cjs_bz_tally* out, size_t cap, cjs_bz_tally_info* info, const cjs_opts* opts, const std::vector<uint32_t>& touched, int dev) {
  const uint64_t nwin = end - first;
  size_t bound = 1;
  for (uint32_t b : touched) bound += idx->e[b].size;
  const size_t work = text_keys_work_bytes(bound, LK_PIECE), max_groups = (size_t)std::min<uint64_t>(cap, nwin);
  DevBuf d_stream(in ? std::max<size_t>(n, 1) : 1), d_text(bound), d_keys(sizeof(cjs_bz_linekey) * ((size_t)nwin + 1)), d_work(work),
         d_stage(sizeof(cjs_bz_tally) * std::max<size_t>(max_groups, 1));
  Arena arena;
  TallyWork w;
  if (!d_stream.p || !d_text.p || !d_keys.p || !d_work.p || !d_stage.p) return CJS_E_OUT_OF_MEMORY;
  CJS_TRY(arena.init_pooled(TallyWork::bytes_needed((size_t)nwin)));
  CJS_TRY(w.carve(arena, (size_t)nwin));
  uint64_t h2d = 0, d2h = 0;
  if (in) {
    if (hipMemcpy(d_stream.p, in, n, hipMemcpyHostToDevice) != hipSuccess) return CJS_E_HIP;
    h2d += n;
  }
  cjs_opts here{};                                          // the cut runs on the device this call has selected
  here.struct_size = sizeof here; here.device = dev;
  cjs_bz_cut_info ci;
  size_t text_n = 0;
  const int crc = cjs_bzip2_cut_device(in ? (const uint8_t*)d_stream.p : d_in, n, idx, t, first, count, mode, delim, sel, nsel, (uint8_t*)d_text.p, bound, &text_n,
                                       &ci, &here);
  info->blocks_decoded = ci.blocks_decoded; info->n_bad_blocks = ci.n_bad_blocks; info->first_bad_block = ci.first_bad_block;
  if (crc) return crc;                                      // (with the cut's detail)
  Stream s;
  CJS_HIP_TRY(hipStreamCreate(s.put()));
  uint64_t nkeys = 0;
  CJS_TRY(text_keys_device(s, (const uint8_t*)d_text.p, text_n, lk_bases(seed), LK_PIECE, true, (cjs_bz_linekey*)d_keys.p, (size_t)nwin + 1, (uint8_t*)d_work.p, &nkeys,
                           &h2d, &d2h));
  cjs_tally_info ti{nkeys, 0, 0, 0, 0};
  if (nkeys) CJS_TRY(tally_to_host(s, w, (const cjs_bz_linekey*)d_keys.p, (uint32_t)nkeys, order, min_count, max_count, first, out, cap, &ti, (cjs_bz_tally*)d_stage.p));
  info->n_lines = nkeys; info->n_bad_lines = ti.n_bad; info->n_distinct = ti.n_distinct; info->n_groups = ti.n_groups; info->max_count = ti.max_count;
  if (env_debug())
    fprintf(stderr, "[cjs tally] %s: lines [%llu, %llu), mode %s, %zu of %zu blocks touched, %zu text bytes in %zu pieces, %llu distinct, %llu kept, beyond the cut: "
            "H2D %llu D2H %llu\n", d_in ? "device" : "host", (unsigned long long)first, (unsigned long long)end, mode == CJS_CUT_FIELDS ? "fields" : "bytes", touched.size(),
            idx->e.size(), text_n, text_keys_pieces(text_n, LK_PIECE), (unsigned long long)ti.n_distinct, (unsigned long long)ti.n_groups, (unsigned long long)h2d,
            (unsigned long long)(d2h + 8 * TL_SCALARS + sizeof(cjs_bz_tally) * std::min<uint64_t>(cap, ti.n_groups)));
  return 0;
}

// cjs_bzip2_tally[_device]: the passes of line_keys_core with the records kept in a device array of the window's lines, then the
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
  const uint64_t N = t->cum.back();
  const uint64_t end = first + count < first ? N + 1 : std::min(first + count, N + 1);      // (the add saturates)
  if (first >= end) return 0;
  const uint64_t nwin = end - first;
  if (nwin > std::min<uint64_t>(max_lines, TL_MAX_KEYS)) return CJS_E_UNSUPPORTED;
  const std::vector<uint32_t> touched = window_blocks(idx, t, first, end);
  info->blocks_decoded = touched.size();
  if (touched.empty()) return 0;      // a stream without a block: its one line is the empty tail, which is no line
  CallDevice cd;
  CJS_TRY(cd.select(opts));
  if (d_in && !on_device(d_in, cd.dev)) return CJS_E_INVALID_ARG;      // (no host pointer reaches a kernel)
  if (mode != CJS_TALLY_LINES)
    return tally_cut(in, d_in, n, idx, t, first, end, count, seed, mode, delim, sel, nsel, order, min_count, max_count, out, cap, info, opts, touched, cd.dev);
  DevBuf d_keys(sizeof(cjs_bz_linekey) * (size_t)nwin);
  Arena arena;
  TallyWork w;
  if (!d_keys.p) return CJS_E_OUT_OF_MEMORY;
  CJS_TRY(arena.init_pooled(TallyWork::bytes_needed((size_t)nwin)));
  CJS_TRY(w.carve(arena, (size_t)nwin));
  // ... and the patches (at most one per touched block, and the tail) and the groups on their way down
  const size_t max_patches = touched.size() + 1, max_groups = (size_t)std::min<uint64_t>(cap, nwin);
  DevBuf d_patch(sizeof(LkPatch) * max_patches), d_stage(sizeof(cjs_bz_tally) * std::max<size_t>(max_groups, 1));
  if (!d_patch.p || !d_stage.p) return CJS_E_OUT_OF_MEMORY;
  LineKeysCall C;
  C.ix = idx; C.t = t;
  C.J.t = t; C.J.B = lk_bases(seed); C.J.first = first; C.J.end = end; C.J.cap = (size_t)nwin; C.J.touched = &touched;
  C.J.d_keys = (cjs_bz_linekey*)d_keys.p;
  RangeStats st;
  RangeVerdicts V(idx);
  CJS_TRY(range_engine(in, d_in, idx, touched, V, cd.dev, st, [&](const RangeBatch& B) { return C.batch(B); }));
  C.J.finish();
  const BadBlocks bad = V.bad_among(touched);
  info->n_bad_blocks = bad.n; info->first_bad_block = bad.first;
  // every pass has drained its stream: the fills, the patches and the grouping go on one of their own
  Stream s;
  CJS_HIP_TRY(hipStreamCreate(s.put()));
  for (const auto& f : C.J.fills) dev_fill(s, C.J.d_keys + f.first, 0xFF, sizeof(cjs_bz_linekey) * (size_t)(f.second - f.first));
  const size_t np = C.J.patches.size();
  int rc = np > max_patches ? (int)CJS_E_HIP : 0;      // (cannot be: a patch per block with a newline, and the tail)
  if (!rc && np) {
    if (hipMemcpyAsync(d_patch.p, C.J.patches.data(), sizeof(LkPatch) * np, hipMemcpyHostToDevice, s) != hipSuccess) rc = CJS_E_HIP;
    else hipLaunchKernelGGL(lk_patch, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, s, C.J.d_keys, (const LkPatch*)d_patch.p, (uint32_t)np);
  }
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

// cjs_bzip2_sort[_device], a composition in the manner of tally_cut: cjs_bzip2_cut_device into a pooled buffer of
// the touched blocks' bytes + 1 (whole lines: the cut with bytes 1-), then the line sort of that text (sort.hip), line numbers
// raised by the window's first.  Everything is sized from the tables and taken before the cut runs.  lines_out / counts_out are
// host memory; the text goes to *text_out (host form: allocated here) or to d_text_out.
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
  const uint64_t N = t->cum.back();
  const uint64_t end = first + count < first ? N + 1 : std::min(first + count, N + 1);      // (the add saturates)
  const std::vector<uint32_t> touched = first < end ? window_blocks(idx, t, first, end) : std::vector<uint32_t>();
  info->blocks_decoded = touched.size();
  if (touched.empty()) {      // an empty window, or a stream without a block: its one line is the empty tail, which is no line
    if (text_out && !(*text_out = HostBuf(1).release())) return CJS_E_OUT_OF_MEMORY;
    return 0;
  }
  const uint64_t nwin = end - first;
  uint64_t bytes = 0;
  for (uint32_t b : touched) bytes += idx->e[b].size;
  if (bytes > std::min<uint64_t>(max_bytes, SL_MAX_BYTES) || nwin > std::min<uint64_t>(max_lines, SL_MAX_LINES)) return CJS_E_UNSUPPORTED;
  const size_t bound = (size_t)bytes + 1, room = (size_t)std::min<uint64_t>(cap, nwin);
  CallDevice cd;
  CJS_TRY(cd.select(opts));
  if (d_in && !on_device(d_in, cd.dev)) return CJS_E_INVALID_ARG;      // (no host pointer reaches a kernel)
  if (d_text_out && !on_device(d_text_out, cd.dev)) return CJS_E_INVALID_ARG;
  DevBuf d_stream(in ? std::max<size_t>(n, 1) : 1), d_text(bound), d_lines(8 * std::max<size_t>(room, 1)), d_counts(counts_out ? 8 * std::max<size_t>(room, 1) : 8),
         d_out(text_out ? bound : 1);
  Arena ca, wa;
  SortCount c;
  SortWork w;
  if (!d_stream.p || !d_text.p || !d_lines.p || !d_counts.p || !d_out.p) return CJS_E_OUT_OF_MEMORY;
  CJS_TRY(ca.init_pooled(SortCount::bytes_needed(bound)));
  CJS_TRY(c.carve(ca, bound));
  CJS_TRY(wa.init_pooled(SortWork::bytes_needed((size_t)nwin)));
  CJS_TRY(w.carve(wa, (size_t)nwin));
  SortStats st;
  if (in) {
    if (hipMemcpy(d_stream.p, in, n, hipMemcpyHostToDevice) != hipSuccess) return CJS_E_HIP;
    st.h2d += n;
  }
  cjs_opts here{};                                          // the cut runs on the device this call has selected
  here.struct_size = sizeof here; here.device = cd.dev;
  cjs_bz_cut_info ci;
  size_t cut_n = 0;
  const int crc = cjs_bzip2_cut_device(in ? (const uint8_t*)d_stream.p : d_in, n, idx, t, first, count, mode, delim, sel, nsel, (uint8_t*)d_text.p, bound, &cut_n, &ci,
                                       &here);
  info->blocks_decoded = ci.blocks_decoded; info->n_bad_blocks = ci.n_bad_blocks; info->first_bad_block = ci.first_bad_block;
  if (crc) return crc;                                      // (with the cut's detail)
  Stream s;
  CJS_HIP_TRY(hipStreamCreate(s.put()));
  const SortStats cut_st = st;
  st = SortStats();
  uint64_t L = 0;
  if (cut_n) CJS_TRY(sort_count(s, c, (const uint8_t*)d_text.p, cut_n, &L, st));
  if (L > nwin) return CJS_E_HIP;                           // (cannot be: the cut writes a line per line of the window at most)
  int rc = 0;
  size_t tn = 0;
  if (L) {
    SortCall q;
    q.d_text = (const uint8_t*)d_text.p; q.n = cut_n; q.flags = flags; q.base = first; q.d_lines = (uint64_t*)d_lines.p;
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
            "beyond the cut: H2D %llu D2H %llu\n", d_in ? "device" : "host", (unsigned long long)first, (unsigned long long)end, touched.size(), idx->e.size(), cut_n,
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

// EXISTS FOR TESTS: the keys of the lines of plain text in device memory, by the middle step of the tally of a cut, brought down.
extern "C" int cjs_stage_text_keys_device(const uint8_t* d_text, size_t n, uint64_t seed, cjs_bz_linekey* keys, size_t cap, size_t* n_lines, size_t piece_bytes,
                                          const cjs_opts* opts) {
  CJS_GUARD_BEGIN
  clear_detail();
  if ((!d_text && n) || (!keys && cap) || !n_lines) return CJS_E_INVALID_ARG;
  const size_t piece = piece_bytes ? piece_bytes : LK_PIECE;
  if (piece > 0x7FFFFFFFu) return CJS_E_INVALID_ARG;
  CallDevice cd;
  CJS_TRY(cd.select(opts));
  if (n && !on_device(d_text, cd.dev)) return CJS_E_INVALID_ARG;      // (no host pointer reaches a kernel)
  // a first run of the summaries alone would give the lines; the hook takes room for the most there can be instead: a line a byte
  const size_t room = n + 1;
  DevBuf d_keys(sizeof(cjs_bz_linekey) * room), d_work(text_keys_work_bytes(n, piece));
  if (!d_keys.p || !d_work.p) return CJS_E_OUT_OF_MEMORY;
  Stream s;
  CJS_HIP_TRY(hipStreamCreate(s.put()));
  uint64_t nk = 0;
  CJS_TRY(text_keys_device(s, d_text, n, lk_bases(seed), piece, false, (cjs_bz_linekey*)d_keys.p, room, (uint8_t*)d_work.p, &nk, nullptr, nullptr));
  *n_lines = (size_t)nk;
  const size_t m = std::min<size_t>(cap, (size_t)nk);
  if (m && hipMemcpy(keys, d_keys.p, sizeof(cjs_bz_linekey) * m, hipMemcpyDeviceToHost) != hipSuccess) return CJS_E_HIP;
  return 0;
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

extern "C" int cjs_bzip2_line_keys(const uint8_t* in, size_t n, const cjs_bz_index* idx, const cjs_bz_lines* lines, uint64_t first, uint64_t count, uint64_t seed,
                                   cjs_bz_linekey* keys, size_t cap, cjs_bz_linekeys_info* info, const cjs_opts* opts) {
  CJS_GUARD_BEGIN
  if (!in && n) return CJS_E_INVALID_ARG;
  return line_keys_core(in ? in : (const uint8_t*)"", nullptr, n, idx, lines, first, count, seed, keys, cap, info, opts);
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

extern "C" int cjs_bzip2_line_keys_device(const uint8_t* d_in, size_t n, const cjs_bz_index* idx, const cjs_bz_lines* lines, uint64_t first, uint64_t count,
                                          uint64_t seed, cjs_bz_linekey* keys, size_t cap, cjs_bz_linekeys_info* info, const cjs_opts* opts) {
  CJS_GUARD_BEGIN
  if (!d_in && n) return CJS_E_INVALID_ARG;
  return line_keys_core(nullptr, d_in, n, idx, lines, first, count, seed, keys, cap, info, opts);
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

extern "C" int cjs_stage_line_keys(const uint8_t* text, size_t n, uint64_t seed, cjs_bz_linekey* keys, size_t cap, size_t* n_lines) {
  if ((!text && n) || (!keys && cap) || !n_lines) return CJS_E_INVALID_ARG;
  *n_lines = lk_text_keys(text, n, seed, keys, cap);
  return 0;
}

extern "C" int cjs_line_keys_diff(const cjs_bz_linekey* a, size_t na, const cjs_bz_linekey* b, size_t nb, uint64_t max_edits, cjs_bz_hunk* hunks, size_t cap,
                                  cjs_bz_ldiff_info* info) {
  if (!info || (!a && na) || (!b && nb) || (!hunks && cap)) return CJS_E_INVALID_ARG;
  CJS_GUARD_BEGIN
  return lk_diff(a, na, b, nb, max_edits, hunks, cap, info);
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_INVALID_ARG)
}
