// linekeys.hip -- a key per line of an indexed .bz2 stream (cjs_bzip2_line_keys[_device]): the sixth consumer of the
// pass engine of the indexed entry points (range_engine.h).  Every decoded inverse-BWT batch is hashed where it stands expanded
// in device scratch; 16 bytes per newline and 32 per block leave the GPU.
//   lk_summary  per 16 KiB tile of a block: the number of newlines in it, the fragment behind its last newline
//   lk_chain    per block: the exclusive scan of its tile counts and its total; the tiles' fragments chained into every tile's
//               carry-in (the fragment between the block's last newline in front of the tile and the tile); the block's tail
//   lk_emit     per tile again: a record per newline at rank = the tile's scanned count + the rank in the tile
// cjs_bzip2_tally[_device] (tally_stream.hip) runs the same passes with a second destination: the records stay in a
// device array of the window's lines (lk_heads brings down a block's first record alone, lk_patch puts the joined ones up).
// The arithmetic of the key is line_key.h, the records, the workspace and the join are line_join.h, the line diff over the keys is
// line_diff.h (all without HIP); linekeys.h is what the tally and the sort of a stream (sort_stream.hip) take from here.
// Tile geometry is that of lines.hip (ln_count / ln_scan, restated here with the hash beside the count): a tile never spans two
// blocks.  A thread takes a contiguous share of its tile's 16-byte vectors (4 or 5 of them) and walks it byte by byte, two
// Horner steps a byte; the shares are joined by a segmented scan (a share with a newline cuts what stands in front of it off).
#include "linekeys.h"
#include "line_diff.h"
#include <algorithm>
#include <numeric>
#include <string.h>

using namespace cjs;

namespace cjs {

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
__global__ __launch_bounds__(256) void lk_patch(cjs_bz_linekey* __restrict__ keys, const LkPatch* __restrict__ p, uint32_t np) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < np) keys[p[i].at] = p[i].key;
}

}  // namespace cjs

// ---------------------------------------------------------------- the pass and its callers
namespace {

// The first half of a key pass over blks in nt tiles, on stream s: the blocks up, lk_summary, lk_chain, the blocks' newline totals
// down into tot.  Returns with s drained.
int lk_pass_count(hipStream_t s, const LkMem& m, const std::vector<LkBlk>& blks, uint64_t nt, const LkBases& B, uint32_t* tot) {
  const size_t nblk = blks.size(); int rc = 0;
  // from here on no way out without a synchronize: the copies may still be reading or writing the vectors
  if (hipMemcpyAsync(m.blk, blks.data(), sizeof(LkBlk) * nblk, hipMemcpyHostToDevice, s) != hipSuccess) rc = CJS_E_HIP;
  else {
    hipLaunchKernelGGL(lk_summary, dim3((unsigned)nt), dim3(256), 0, s, (const LkBlk*)m.blk, (uint32_t)nblk, B, m.cnt, m.open);
    hipLaunchKernelGGL(lk_chain, dim3((unsigned)nblk), dim3(256), 0, s, (const LkBlk*)m.blk, B, m.cnt, m.open, m.tot, m.tail);
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(tot, m.tot, 4 * nblk, hipMemcpyDeviceToHost, s) != hipSuccess) rc = CJS_E_HIP;
  }
  return drained(s, rc);
}
// The second half, once every block's nrec on the device is its total: lk_emit writes the records to d_out, between() queues what the caller
// does with them there, lk_heads if `heads`; the tails come down, and n_down records from the heads or else from d_out.  rc: of what
// the caller has queued in front (not 0: nothing more is).  Returns with s drained.
template <typename F>
int lk_pass_emit(hipStream_t s, const LkMem& m, size_t nblk, uint64_t nt, const LkBases& B, cjs_bz_linekey* d_out, bool heads, LkTail* tails, cjs_bz_linekey* down,
                 size_t n_down, int rc, F between) {
  if (!rc) {
    hipLaunchKernelGGL(lk_emit, dim3((unsigned)nt), dim3(256), 0, s, (const LkBlk*)m.blk, (uint32_t)nblk, B, (const uint32_t*)m.cnt, (const LkOpen*)m.open, d_out, m.tail);
    rc = between();
    if (heads) hipLaunchKernelGGL(lk_heads, dim3((unsigned)((nblk + 255) / 256)), dim3(256), 0, s, (const LkBlk*)m.blk, (uint32_t)nblk, (const cjs_bz_linekey*)d_out, m.head);
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(tails, m.tail, sizeof(LkTail) * nblk, hipMemcpyDeviceToHost, s) != hipSuccess ||
        (n_down && hipMemcpyAsync(down, heads ? m.head : d_out, sizeof(cjs_bz_linekey) * n_down, hipMemcpyDeviceToHost, s) != hipSuccess)) rc = CJS_E_HIP;
  }
  return drained(s, rc);
}

int line_keys_core(const uint8_t* in, const uint8_t* d_in, size_t n, const cjs_bz_index* idx, const cjs_bz_lines* t, uint64_t first, uint64_t count,
                   uint64_t seed, cjs_bz_linekey* keys, size_t cap, cjs_bz_linekeys_info* info, const cjs_opts* opts) {
  clear_detail();
  if (!idx || !t || !info || (!keys && cap)) return CJS_E_INVALID_ARG;
  CJS_TRY(check_index_stream(in ? in : d_in, n, idx));
  if (!lines_belong(idx, t)) return CJS_E_INVALID_ARG;
  info->n_lines = info->n_bad_blocks = info->blocks_decoded = 0; info->first_bad_block = ~0ull;
  const uint64_t end = line_window_end(first, count, t->cum.back());
  if (first >= end) return 0;
  info->n_lines = end - first;
  if (!cap) return 0;                                              // the count query: the table alone
  const std::vector<uint32_t> touched = line_window_blocks(t->cum, t->total_bytes, idx->off, first, end);
  LineKeysCall C(idx, t, seed, first, end, touched);
  C.J.keys = keys; C.J.cap = cap;
  RangeStats st; RangeVerdicts V(idx);
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

// A decoded batch: a pass over its good blocks, their fragments into the join.  The records come down whole, or for the tally they
// go to their ranks in J.d_keys and the first one of every block comes down.
int LineKeysCall::batch(const RangeBatch& B) {
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
  const LkLayout L(nblk, (size_t)nt, (size_t)nrec, J.d_keys != nullptr);
  DevBuf mem(L.bytes);
  if (!mem.p) return CJS_E_OUT_OF_MEMORY;
  const LkMem m((uint8_t*)mem.p, L);
  std::vector<uint32_t> tot(nblk); std::vector<LkTail> tails(nblk);
  // what comes down: every record, or for the tally the first one of every block (pinned from 1 MiB on: the records of 100 MB of text are 14 MB)
  const size_t down = J.d_keys ? nblk : (size_t)nrec;
  HostBuf staged(sizeof(cjs_bz_linekey) * std::max<size_t>(down, 1));
  if (!staged.p) return CJS_E_OUT_OF_MEMORY;
  cjs_bz_linekey* recs = (cjs_bz_linekey*)staged.p;
  hipStream_t s = B.s;
  CJS_TRY(lk_pass_count(s, m, blks, nt, J.B, tot.data()));
  // the records are written at the table's ranks: only over blocks that have the table's newlines
  for (size_t i = 0; i < nblk; i++)
    if (tot[i] != blks[i].nrec) { set_detail("line table does not match the stream at block %u", which[i]); return CJS_E_DATA_ERROR; }
  CJS_TRY(lk_pass_emit(s, m, nblk, nt, J.B, m.rec, J.d_keys != nullptr, tails.data(), recs, down, 0, [&] {
    if (!J.d_keys) return 0;
    // the records of the window go to their ranks in the device array, a copy per run of blocks whose ranks follow one another
    // (the first record of a block is not yet its line's key: the join's patch follows at the end)
    int rc = 0;
    uint64_t run_dst = 0, run_src = 0, run_n = 0;
    auto flush = [&] {
      if (run_n && hipMemcpyAsync(J.d_keys + run_dst, m.rec + run_src, sizeof(cjs_bz_linekey) * (size_t)run_n, hipMemcpyDeviceToDevice, s) != hipSuccess) rc = CJS_E_HIP;
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
    return rc;
  }));
  h2d += sizeof(LkBlk) * nblk; d2h += 4 * nblk + sizeof(LkTail) * nblk + sizeof(cjs_bz_linekey) * down; tiles += nt;
  for (size_t i = 0; i < nblk; i++) J.good(which[i], recs + (J.d_keys ? i : blks[i].rec0), tails[i]);
  return 0;
}

int cjs::lk_apply_join(hipStream_t s, const LkJoin& J, LkPatch* d_patch, size_t max_patches) {
  for (const auto& f : J.fills) dev_fill(s, J.d_keys + f.first, 0xFF, sizeof(cjs_bz_linekey) * (size_t)(f.second - f.first));
  const size_t np = J.patches.size();
  if (np > max_patches) return CJS_E_HIP;                   // (cannot be: a patch per block or piece with a newline, and the tail)
  if (!np) return 0;
  if (hipMemcpyAsync(d_patch, J.patches.data(), sizeof(LkPatch) * np, hipMemcpyHostToDevice, s) != hipSuccess) return CJS_E_HIP;
  hipLaunchKernelGGL(lk_patch, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, s, J.d_keys, (const LkPatch*)d_patch, (uint32_t)np);
  return hipGetLastError() != hipSuccess ? (int)CJS_E_HIP : 0;
}

// ---- the keys of the lines of plain text in device memory (the tally of a cut; cjs_stage_text_keys_device)
// The text is cut into pieces of at most `piece` bytes, and the kernels see a piece as they see a block: lk_summary and lk_chain
// over all pieces at once, the pieces' totals come down and set rec0 / nrec (a piece's record count is not known before), lk_emit
// writes the records at their ranks straight into d_keys, lk_heads brings the first record of every piece down, and the same LkJoin
// that joins blocks joins the pieces over a table made of those totals: a patch per piece with a newline, and the tail.
int cjs::text_keys_device(hipStream_t s, const uint8_t* d_text, size_t n, const LkBases& B, size_t piece, bool tally_tail, cjs_bz_linekey* d_keys, size_t key_cap,
                          uint8_t* d_work, uint64_t* n_keys, uint64_t* h2d, uint64_t* d2h) {
  const size_t np = text_keys_pieces(n, piece);
  std::vector<LkBlk> blks(np);
  uint64_t nt = 0;
  for (size_t i = 0; i < np; i++) {
    const uint32_t len = (uint32_t)std::min(piece, n - i * piece);
    blks[i] = LkBlk{(uint64_t)(uintptr_t)(d_text + i * piece), 0, len, (uint32_t)nt, 0, (uint32_t)i};
    nt += lk_tiles(len);
  }
  if (nt > 0x7FFFFFFFull || np > 0x7FFFFFFFull) return drained(s, CJS_E_UNSUPPORTED);
  const LkLayout L(np, (size_t)nt, 0, true);
  const LkMem m(d_work, L);
  LkPatch* d_patch = (LkPatch*)(d_work + L.bytes);
  std::vector<uint32_t> tot(np); std::vector<LkTail> tails(np); std::vector<cjs_bz_linekey> heads(np);
  cjs_bz_lines table;                                       // the pieces' newlines as a line table: what LkJoin reads of one
  table.cum.assign(1, 0);
  if (np) {
    CJS_TRY(lk_pass_count(s, m, blks, nt, B, tot.data()));
    for (size_t i = 0; i < np; i++) {
      blks[i].rec0 = table.cum.back(); blks[i].nrec = tot[i];
      table.nl.push_back(tot[i]); table.cum.push_back(table.cum.back() + tot[i]);
    }
  }
  const uint64_t total = table.cum.back();
  if (total >= key_cap) return CJS_E_HIP;                   // (cannot be: the caller's room is the lines of the text, and one for the tail)
  std::vector<uint32_t> all(np);
  std::iota(all.begin(), all.end(), 0u);
  LkJoin J;
  J.t = &table; J.B = B; J.first = 0; J.end = total + 1; J.cap = (size_t)total + 1; J.touched = &all; J.d_keys = d_keys; J.tally_tail = tally_tail;
  if (np) {
    const int up = hipMemcpyAsync(m.blk, blks.data(), sizeof(LkBlk) * np, hipMemcpyHostToDevice, s) != hipSuccess ? (int)CJS_E_HIP : 0;
    CJS_TRY(lk_pass_emit(s, m, np, nt, B, d_keys, true, tails.data(), heads.data(), np, up, [] { return 0; }));
    for (size_t i = 0; i < np; i++) J.good((uint32_t)i, &heads[i], tails[i]);
  }
  J.finish();
  const int rc = lk_apply_join(s, J, d_patch, np + 1);
  *n_keys = total + 1 - (J.tail_dropped ? 1 : 0);
  if (h2d) *h2d += 2 * sizeof(LkBlk) * np + sizeof(LkPatch) * J.patches.size();
  if (d2h) *d2h += (4 + sizeof(LkTail) + sizeof(cjs_bz_linekey)) * np;
  return drained(s, rc);
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
