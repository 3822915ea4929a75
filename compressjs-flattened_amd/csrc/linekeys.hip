// linekeys.hip -- a key per line of an indexed .bz2 stream (cjs_bzip2_line_keys[_device]): the sixth consumer of the
// pass engine of the indexed entry points (range_engine.h).  Every decoded inverse-BWT batch is hashed where it stands expanded
// in device scratch; 16 bytes per newline and 32 per block leave the GPU.
//   lk_summary  per 16 KiB tile of a block: the number of newlines in it, the fragment behind its last newline
//   lk_chain    per block: the exclusive scan of its tile counts and its total; the tiles' fragments chained into every tile's
//               carry-in (the fragment between the block's last newline in front of the tile and the tile); the block's tail
//   lk_emit     per tile again: a record per newline at rank = the tile's scanned count + the rank in the tile
// The arithmetic of the key and of the join is line_key.h; the line diff over the keys is line_diff.h (both without HIP).
// Tile geometry is that of lines.hip (ln_count / ln_scan, restated here with the hash beside the count): a tile never spans two
// blocks.  A thread takes a contiguous share of its tile's 16-byte vectors (4 or 5 of them) and walks it byte by byte, two
// Horner steps a byte; the shares are joined by a segmented scan (a share with a newline cuts what stands in front of it off).
#include "range_engine.h"
#include "bz_lines.h"
#include "line_key.h"
#include "line_diff.h"
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

  void put(uint64_t line, const cjs_bz_linekey& k) { if (line >= first && line < end && line - first < cap) keys[line - first] = k; }
  // a touched block that did not come as a good one: its lines, the one that goes on behind it included
  void bad(uint32_t b) {
    for (uint64_t k = t->cum[b]; k < t->cum[b + 1]; k++) put(k, lk_bad_key());
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
    if (lo < hi) memcpy(keys + (lo - first), recs + (lo - l0), sizeof(cjs_bz_linekey) * (size_t)(hi - lo));
    open = behind; open_bad = false;
  }
  void finish() {
    while (at < touched->size()) bad((*touched)[at++]);
    put(t->cum.back(), open_bad ? lk_bad_key() : lk_key(open));      // the tail line (inside the window iff the last block was touched)
  }
};

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
                 o_tail = o_tot + pad(4 * nblk), o_rec = o_tail + pad(sizeof(LkTail) * nblk), bytes = o_rec + pad(sizeof(cjs_bz_linekey) * (size_t)nrec);
    DevBuf mem(bytes);
    if (!mem.p) return CJS_E_OUT_OF_MEMORY;
    uint8_t* d = (uint8_t*)mem.p;
    LkBlk* d_blk = (LkBlk*)(d + o_blk); uint32_t* d_cnt = (uint32_t*)(d + o_cnt); LkOpen* d_open = (LkOpen*)(d + o_open);
    uint32_t* d_tot = (uint32_t*)(d + o_tot); LkTail* d_tail = (LkTail*)(d + o_tail); cjs_bz_linekey* d_rec = (cjs_bz_linekey*)(d + o_rec);
    std::vector<uint32_t> tot(nblk); std::vector<LkTail> tails(nblk);
    HostBuf staged(sizeof(cjs_bz_linekey) * (size_t)std::max<uint64_t>(nrec, 1));      // (pinned from 1 MiB on: the records of 100 MB of text are 14 MB)
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
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(tails.data(), d_tail, sizeof(LkTail) * nblk, hipMemcpyDeviceToHost, s) != hipSuccess ||
        (nrec && hipMemcpyAsync(recs, d_rec, sizeof(cjs_bz_linekey) * (size_t)nrec, hipMemcpyDeviceToHost, s) != hipSuccess)) rc = CJS_E_HIP;
    CJS_TRY(drained(s, rc));
    h2d += sizeof(LkBlk) * nblk; d2h += 4 * nblk + sizeof(LkTail) * nblk + sizeof(cjs_bz_linekey) * (size_t)nrec; tiles += nt;
    for (size_t i = 0; i < nblk; i++) J.good(which[i], recs + blks[i].rec0, tails[i]);
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
  // from the block of newline number `first` through the block of newline number `end`, the line table's routing of a line's start
  std::vector<uint32_t> touched;
  if (!idx->e.empty()) {
    const LineRoute r0 = route_locate(t->cum, t->total_bytes, first), r1 = route_locate(t->cum, t->total_bytes, end);
    const size_t b0 = first ? r0.block : 0, b1 = end <= N ? r1.block : idx->e.size() - 1;
    for (size_t b = b0; b <= b1; b++) if (idx->e[b].size) touched.push_back((uint32_t)b);
  }
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

}  // namespace

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
