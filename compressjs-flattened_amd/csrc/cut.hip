// cut.hip -- fields or byte columns of the lines of an indexed .bz2 stream (cjs_bzip2_cut[_device]): the seventh
// consumer of the pass engine of the indexed entry points (range_engine.h).  Every decoded inverse-BWT batch is cut where it stands
// expanded in device scratch; only the selected bytes leave the GPU.
//   ct_summary  per 16 KiB tile of a block: its summary (newlines; units and "any byte" behind the last of them)
//   ct_chain    one workgroup over all tiles of the batch: the summaries composed from the batch's carry-in (the state the batch or
//               pass in front left) into every tile's carry-in; the line number checked against the table at both ends of every
//               block; the batch's carry-out
//   ct_count    per tile: the bytes it writes, from its carry-in and the window
//   ct_scan     the exclusive prefix sums of the counts and their total
//   ct_emit     per tile again: every thread ranks its bytes by the workgroup's prefix sums, the tile's output is packed in LDS at
//               the phase of its destination and stored with 16-byte vectors where a whole one is inside, bytes at the two ends
// The arithmetic (selection, summary, monoid, emit rule) is cut_plan.h, without HIP; tally_stream.hip and sort_stream.hip take the cut
// as device text (linekeys.h).  Tile geometry is that of lines.hip and linekeys.hip: a tile never spans two blocks; a thread takes a
// contiguous share of its tile's 16-byte vectors (4 or 5) and walks it byte by byte; the shares are joined by a scan of their summaries.
// No atomics decide an order.
#include "range_engine.h"
#include "bz_lines.h"
#include "cut_plan.h"
#include <algorithm>
#include <stdlib.h>
#include <string.h>

using namespace cjs;

namespace cjs {

constexpr uint32_t CT_TILE = 16384;                        // bytes of a tile: that of the line table
struct CtBlk { uint64_t src, line0; uint32_t len, tile0, nl, blk; };      // len bytes at src; its first byte's line number and its newlines by the table
struct CtRes { CtSum carry; uint64_t total; uint32_t bad, pad; };         // of a batch: the state behind it, the bytes it writes, the first block off the table (~0: none)
struct CtWin { uint64_t first, end; };                                     // the window, as line numbers

__host__ __device__ __forceinline__ uint32_t ct_tiles(uint32_t len) { return (len + CT_TILE - 1) / CT_TILE; }

__device__ __forceinline__ CtSum ct_shfl_up(const CtSum& e, int d) { return CtSum{__shfl_up(e.nl, d, 64), __shfl_up(e.units, d, 64), __shfl_up(e.flags, d, 64)}; }
// Workgroup of 256: the composition of the summaries in front of this thread's, `total` = of all of them.  sm: four summaries.
__device__ __forceinline__ CtSum ct_block_excl(const CtSum& v, CtSum* sm, CtSum& total) {
  CtSum x = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const CtSum y = ct_shfl_up(x, d);
    if (lane_id() >= d) x = ct_comb(y, x);
  }
  if (lane_id() == 63) sm[wave_id()] = x;
  CtSum prev = ct_shfl_up(x, 1);
  if (lane_id() == 0) prev = ct_none();
  __syncthreads();
  CtSum base = ct_none();
  total = ct_none();
  for (int w = 0; w < 4; w++) {
    if (w == wave_id()) base = total;
    total = ct_comb(total, sm[w]);
  }
  __syncthreads();
  return ct_comb(base, prev);
}

// f(byte) for every byte of the tile in vectors [v0, v1) of its span, in order (a vector's bytes outside the tile are left out)
template <typename F>
__device__ __forceinline__ void ct_bytes(const RgSpan& S, uint32_t v0, uint32_t v1, F f) {
  const uint64_t end = S.a0 + S.n;
  for (uint32_t v = v0; v < v1; v++) {
    const uint64_t a = S.base + 16ull * v;
    const uint4 x = rg_vec(S, v);
    const uint32_t w[4] = {x.x, x.y, x.z, x.w};
    const uint32_t lo = a < S.a0 ? (uint32_t)(S.a0 - a) : 0u, hi = end - a < 16 ? (uint32_t)(end - a) : 16u;
#pragma unroll
    for (uint32_t q = 0; q < 4; q++) {
      uint32_t d = w[q];
      for (uint32_t i = 4 * q; i < 4 * q + 4; i++, d >>= 8) if (i >= lo && i < hi) f((uint8_t)d);
    }
  }
}

struct CtTileOf { CtBlk g; RgSpan S; uint32_t v0, v1; };
// tile t: its block, its span, this thread's share of the span's vectors
__device__ __forceinline__ CtTileOf ct_tile_of(const CtBlk* __restrict__ blks, uint32_t nblk, uint32_t t) {
  CtTileOf T;
  T.g = rg_seg_of(blks, nblk, t);
  const uint32_t p0 = (t - T.g.tile0) * CT_TILE;
  T.S = rg_span(T.g.src + p0, min(CT_TILE, T.g.len - p0));
  const uint32_t per = (T.S.nvec + 255) / 256;
  T.v0 = min(threadIdx.x * per, T.S.nvec); T.v1 = min(T.v0 + per, T.S.nvec);
  return T;
}
__device__ __forceinline__ CtView ct_view_dev(const CtSel* __restrict__ sel) {
  return CtView{sel->mask, sel->mode, sel->delim, sel->min_lo, sel->n - sel->beyond, sel->r + sel->beyond};
}
// the summary of this thread's share
__device__ __forceinline__ CtSum ct_share(const CtTileOf& T, uint32_t mode, uint32_t delim) {
  CtSum s = ct_none();
  ct_bytes(T.S, T.v0, T.v1, [&](uint8_t ch) { ct_push(s, mode, delim, ch); });
  return s;
}

__global__ __launch_bounds__(256) void ct_summary(const CtBlk* __restrict__ blks, uint32_t nblk, uint32_t mode, uint32_t delim, CtSum* __restrict__ sum) {
  __shared__ CtSum sm[4];
  const CtTileOf T = ct_tile_of(blks, nblk, blockIdx.x);
  CtSum total;
  ct_block_excl(ct_share(T, mode, delim), sm, total);
  if (threadIdx.x == 0) sum[blockIdx.x] = total;
}

// One workgroup: in[t] = carry ∘ sum[0] ∘ .. ∘ sum[t - 1] for the nt tiles of the batch, res->carry = behind the last.  The line
// number in front of every block's first tile and behind its last is what the table says, or res->bad = the first such block's
// place in blks (the minimum: whichever thread finds it).
__global__ __launch_bounds__(256) void ct_chain(const CtBlk* __restrict__ blks, uint32_t nblk, uint32_t nt, CtSum carry, const CtSum* __restrict__ sum,
                                                CtSum* __restrict__ in, CtRes* __restrict__ res) {
  __shared__ CtSum sm[4];
  __shared__ uint32_t bad;
  if (threadIdx.x == 0) bad = ~0u;
  __syncthreads();
  for (uint32_t b = 0; b < nt; b += 256) {
    const uint32_t i = b + threadIdx.x;
    const CtSum e = i < nt ? sum[i] : ct_none();
    CtSum total;
    const CtSum st = ct_comb(carry, ct_block_excl(e, sm, total));
    if (i < nt) {
      in[i] = st;
      const CtBlk g = rg_seg_of(blks, nblk, i);
      if ((i == g.tile0 && st.nl != g.line0) || (i == g.tile0 + ct_tiles(g.len) - 1 && st.nl + e.nl != g.line0 + g.nl)) atomicMin(&bad, g.blk);
    }
    carry = ct_comb(carry, total);
  }
  __syncthreads();
  if (threadIdx.x == 0) { res->carry = carry; res->bad = bad; res->pad = 0; }
}

// no line of the tile (state `in` in front of it, summary s) is inside the window
__device__ __forceinline__ bool ct_outside(const CtSum& in, const CtSum& s, const CtWin& W) { return in.nl >= W.end || in.nl + s.nl < W.first; }

__global__ __launch_bounds__(256) void ct_count(const CtBlk* __restrict__ blks, uint32_t nblk, const CtSel* __restrict__ sel, CtWin W, const CtSum* __restrict__ sum,
                                                const CtSum* __restrict__ in, uint64_t* __restrict__ cnt) {
  __shared__ CtSum sm[4];
  __shared__ uint32_t sc[4];
  const CtSum in0 = in[blockIdx.x];
  if (ct_outside(in0, sum[blockIdx.x], W)) { if (threadIdx.x == 0) cnt[blockIdx.x] = 0; return; }
  const CtTileOf T = ct_tile_of(blks, nblk, blockIdx.x);
  const CtView V = ct_view_dev(sel);
  CtSum total;
  CtSum s = ct_comb(in0, ct_block_excl(ct_share(T, V.mode, V.delim), sm, total));      // the state in front of this share
  uint32_t c = 0;
  ct_bytes(T.S, T.v0, T.v1, [&](uint8_t ch) { c += ct_step(V, W.first, W.end, s, ch) ? 1u : 0u; });
  const uint32_t n = block_sum<256, uint32_t>(c, sc);
  if (threadIdx.x == 0) cnt[blockIdx.x] = n;
}

__global__ __launch_bounds__(256) void ct_scan(uint64_t* __restrict__ cnt, uint32_t nt, CtRes* __restrict__ res) {
  __shared__ uint64_t sm[4];
  const uint64_t total = rg_scan_counts(cnt, (uint64_t)nt, sm, [](uint64_t) {});
  if (threadIdx.x == 0) { cnt[nt] = total; res->total = total; }
}

// The tile's written bytes -> out[off0 + cnt[tile] ..), those at or past out[cap] left out.  They are packed in LDS at the phase of
// their destination address, so a 16-byte vector of LDS is a 16-byte aligned vector of the output.
__global__ __launch_bounds__(256) void ct_emit(const CtBlk* __restrict__ blks, uint32_t nblk, const CtSel* __restrict__ sel, CtWin W, const CtSum* __restrict__ in,
                                               const uint64_t* __restrict__ cnt, uint8_t* __restrict__ out, uint64_t off0, uint64_t cap) {
  __shared__ CtSum sm[4];
  __shared__ uint32_t sc[4];
  __shared__ __attribute__((aligned(16))) uint8_t stage[CT_TILE + 16];
  const uint64_t off = off0 + cnt[blockIdx.x];
  const uint32_t mine = (uint32_t)(cnt[blockIdx.x + 1] - cnt[blockIdx.x]);
  if (!mine || off >= cap) return;
  const CtTileOf T = ct_tile_of(blks, nblk, blockIdx.x);
  const CtView V = ct_view_dev(sel);
  CtSum total;
  const CtSum s0 = ct_comb(in[blockIdx.x], ct_block_excl(ct_share(T, V.mode, V.delim), sm, total));
  CtSum s = s0;
  uint32_t c = 0;
  ct_bytes(T.S, T.v0, T.v1, [&](uint8_t ch) { c += ct_step(V, W.first, W.end, s, ch) ? 1u : 0u; });
  uint32_t all;
  uint32_t r = block_excl_sum<256, uint32_t>(c, sc, all);
  const uint64_t dst = (uint64_t)(uintptr_t)out + off;
  const uint32_t phase = (uint32_t)(dst & 15u);
  s = s0;
  ct_bytes(T.S, T.v0, T.v1, [&](uint8_t ch) { if (ct_step(V, W.first, W.end, s, ch) && r < CT_TILE) stage[phase + r++] = ch; });
  __syncthreads();
  const uint64_t left = cap - off;
  const uint32_t both = min(mine, all), keep = both < left ? both : (uint32_t)left, span = phase + keep;      // bytes [phase, span) of stage go out
  uint8_t* base = out + off - phase;                                                                   // (16-byte aligned; nothing in front of out + off is touched)
  for (uint32_t v = threadIdx.x; 16 * v < span; v += 256) {
    const uint32_t lo = max(16 * v, phase), hi = min(16 * v + 16, span);
    if (hi - lo == 16) *reinterpret_cast<uint4*>(base + 16 * v) = *reinterpret_cast<const uint4*>(stage + 16 * v);
    else for (uint32_t i = lo; i < hi; i++) base[i] = stage[i];
  }
}

}  // namespace cjs

// ---------------------------------------------------------------- the driver
namespace {

struct CutCall {
  const cjs_bz_index* ix = nullptr;
  const cjs_bz_lines* t = nullptr;
  const std::vector<uint32_t>* touched = nullptr; size_t at = 0;      // touched blocks in front of `at` have come, all good
  bool holed = false;                                                 // a touched block did not come as a good one: nothing more is cut
  const CtSel* d_sel = nullptr;
  uint32_t mode = 0, delim = 0;
  CtWin W{0, 0};
  CtSum carry = ct_none();                                            // the state behind the batches so far
  // the result: the host form's buffer (grown by the batch), or the device form's d_out[0 .. cap)
  bool host = false;
  uint8_t* h_out = nullptr; size_t h_room = 0;
  uint8_t* d_out = nullptr; uint64_t cap = 0;
  uint64_t written = 0;                                               // bytes of the output so far, also those that found no room
  uint64_t h2d = 0, d2h = 0, tiles = 0; uint32_t batches = 0;

  ~CutCall() { free(h_out); }
  int room(uint64_t more) {                                           // host form: h_out holds written + more bytes
    const uint64_t need = written + more;
    if (need <= h_room) return 0;
    const uint64_t want = std::max<uint64_t>(need, (uint64_t)h_room + h_room / 2);
    uint8_t* p = (uint8_t*)realloc(h_out, (size_t)want);
    if (!p) return CJS_E_OUT_OF_MEMORY;
    h_out = p; h_room = (size_t)want;
    return 0;
  }

  int batch(const RangeBatch& B) {
    std::vector<CtBlk> blks; std::vector<uint32_t> which;
    uint64_t nt = 0;
    for (size_t k = B.g0; k < B.g1 && !holed; k++) {
      const uint32_t b = B.blk[k];
      // the chain runs from one block's last byte into the next one's first: only over the touched blocks in order, all good
      if (at >= touched->size() || (*touched)[at] != b || !B.V.good(b)) { holed = true; break; }
      at++;
      const uint32_t len = ix->e[b].size;
      blks.push_back(CtBlk{B.addr(k), t->cum[b], len, (uint32_t)nt, t->nl[b], (uint32_t)blks.size()});
      which.push_back(b);
      nt += ct_tiles(len);
    }
    if (holed || blks.empty()) return 0;
    if (nt > 0x7FFFFFFEull) return CJS_E_UNSUPPORTED;
    const size_t nblk = blks.size();
    auto pad = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t o_blk = 0, o_sum = o_blk + pad(sizeof(CtBlk) * nblk), o_in = o_sum + pad(sizeof(CtSum) * (size_t)nt), o_cnt = o_in + pad(sizeof(CtSum) * (size_t)nt),
                 o_res = o_cnt + pad(8 * ((size_t)nt + 1)), bytes = o_res + pad(sizeof(CtRes));
    DevBuf mem(bytes);
    if (!mem.p) return CJS_E_OUT_OF_MEMORY;
    uint8_t* d = (uint8_t*)mem.p;
    CtBlk* d_blk = (CtBlk*)(d + o_blk); CtSum* d_sum = (CtSum*)(d + o_sum); CtSum* d_in = (CtSum*)(d + o_in);
    uint64_t* d_cnt = (uint64_t*)(d + o_cnt); CtRes* d_res = (CtRes*)(d + o_res);
    CtRes res;
    hipStream_t s = B.s;
    int rc = 0;
    // from here on no way out without a synchronize: the copies may still be reading or writing the vectors
    if (hipMemcpyAsync(d_blk, blks.data(), sizeof(CtBlk) * nblk, hipMemcpyHostToDevice, s) != hipSuccess) rc = CJS_E_HIP;
    else {
      hipLaunchKernelGGL(ct_summary, dim3((unsigned)nt), dim3(256), 0, s, (const CtBlk*)d_blk, (uint32_t)nblk, mode, delim, d_sum);
      hipLaunchKernelGGL(ct_chain, dim3(1), dim3(256), 0, s, (const CtBlk*)d_blk, (uint32_t)nblk, (uint32_t)nt, carry, (const CtSum*)d_sum, d_in, d_res);
      hipLaunchKernelGGL(ct_count, dim3((unsigned)nt), dim3(256), 0, s, (const CtBlk*)d_blk, (uint32_t)nblk, d_sel, W, (const CtSum*)d_sum, (const CtSum*)d_in, d_cnt);
      hipLaunchKernelGGL(ct_scan, dim3(1), dim3(256), 0, s, d_cnt, (uint32_t)nt, d_res);
      if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&res, d_res, sizeof res, hipMemcpyDeviceToHost, s) != hipSuccess) rc = CJS_E_HIP;
    }
    CJS_TRY(drained(s, rc));
    h2d += sizeof(CtBlk) * nblk; d2h += sizeof res; tiles += nt; batches++;
    if (res.bad != ~0u) { set_detail("line table does not match the stream at block %u", which[std::min<size_t>(res.bad, nblk - 1)]); return CJS_E_DATA_ERROR; }
    carry = res.carry;
    if (host) {
      if (res.total) {
        CJS_TRY(room(res.total));
        DevBuf piece((size_t)res.total);
        if (!piece.p) return CJS_E_OUT_OF_MEMORY;
        hipLaunchKernelGGL(ct_emit, dim3((unsigned)nt), dim3(256), 0, s, (const CtBlk*)d_blk, (uint32_t)nblk, d_sel, W, (const CtSum*)d_in, (const uint64_t*)d_cnt,
                           (uint8_t*)piece.p, (uint64_t)0, res.total);
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(h_out + written, piece.p, (size_t)res.total, hipMemcpyDeviceToHost, s) != hipSuccess) rc = CJS_E_HIP;
        CJS_TRY(drained(s, rc));
        d2h += res.total;
      }
    } else if (res.total && written < cap) {
      hipLaunchKernelGGL(ct_emit, dim3((unsigned)nt), dim3(256), 0, s, (const CtBlk*)d_blk, (uint32_t)nblk, d_sel, W, (const CtSum*)d_in, (const uint64_t*)d_cnt,
                         d_out, written, cap);
      if (hipGetLastError() != hipSuccess) rc = CJS_E_HIP;
      CJS_TRY(drained(s, rc));
    }
    written += res.total;
    return 0;
  }
};

// host form: out / out_n; device form: d_out / out_cap / out_need
int cut_core(const uint8_t* in, const uint8_t* d_in, size_t n, const cjs_bz_index* idx, const cjs_bz_lines* t, uint64_t first, uint64_t count, uint32_t mode,
             uint32_t delim, const cjs_cut_range* sel, uint32_t nsel, uint8_t** out, size_t* out_n, uint8_t* d_out, size_t out_cap, size_t* out_need,
             cjs_bz_cut_info* info, const cjs_opts* opts) {
  clear_detail();
  const bool host = in != nullptr;
  if (!idx || !t || !info || (host ? (!out || !out_n) : (!out_need || (!d_out && out_cap)))) return CJS_E_INVALID_ARG;
  CtSel S;
  CJS_TRY(ct_normalise(mode, delim, sel, nsel, &S));
  CJS_TRY(check_index_stream(host ? in : d_in, n, idx));
  if (!lines_belong(idx, t)) return CJS_E_INVALID_ARG;
  info->n_lines = info->out_bytes = info->n_bad_blocks = info->blocks_decoded = 0; info->first_bad_block = ~0ull;
  const uint64_t end = line_window_end(first, count, t->cum.back());
  CutCall C;
  C.ix = idx; C.t = t; C.host = host; C.mode = S.mode; C.delim = S.delim; C.W = CtWin{first, end}; C.d_out = d_out; C.cap = out_cap;
  const std::vector<uint32_t> touched = line_window_blocks(t->cum, t->total_bytes, idx->off, first, end);
  if (first < end) info->n_lines = end - first;
  C.touched = &touched;
  RangeStats st;
  RangeVerdicts V(idx);
  if (!touched.empty()) {
    CallDevice cd;
    CJS_TRY(cd.select(opts));
    if (d_in && !on_device(d_in, cd.dev)) return CJS_E_INVALID_ARG;      // (no host pointer reaches a kernel)
    if (d_out && !on_device(d_out, cd.dev)) return CJS_E_INVALID_ARG;
    DevBuf dsel(sizeof(CtSel));
    if (!dsel.p) return CJS_E_OUT_OF_MEMORY;
    if (hipMemcpy(dsel.p, &S, sizeof S, hipMemcpyHostToDevice) != hipSuccess) return CJS_E_HIP;
    C.d_sel = (const CtSel*)dsel.p; C.h2d += sizeof S;
    C.carry = CtSum{t->cum[touched[0]], 0, 0};      // a line in front of the window, or the start of the window's first
    CJS_TRY(range_engine(in, d_in, idx, touched, V, cd.dev, st, [&](const RangeBatch& B) { return C.batch(B); }));
    info->blocks_decoded = touched.size();
    const BadBlocks bad = V.bad_among(touched);
    info->n_bad_blocks = bad.n; info->first_bad_block = bad.first;
    if (bad.n) { V.set_bad_detail(idx, (size_t)bad.first); return CJS_E_DATA_ERROR; }
    if (C.holed || C.at != touched.size()) return CJS_E_HIP;             // (cannot happen: every touched block came good and in order)
    if (ct_tail_newline(C.carry, first, end)) {                           // the tail line, not empty, inside the window
      const uint8_t nl = 0x0A;
      if (host) { CJS_TRY(C.room(1)); C.h_out[C.written] = nl; }
      else if (C.written < C.cap) {
        if (hipMemcpy(d_out + C.written, &nl, 1, hipMemcpyHostToDevice) != hipSuccess) return CJS_E_HIP;
        C.h2d++;
      }
      C.written++;
    }
  }
  info->out_bytes = C.written;
  if (env_debug())
    fprintf(stderr, "[cjs cut] %s: lines [%llu, %llu), %zu of %zu blocks touched, %u passes (%u row batches, %u inverse-BWT batches), %u cut batches, %llu tiles, "
            "%llu output bytes, H2D %llu D2H %llu\n", host ? "host" : "device", (unsigned long long)first, (unsigned long long)end, touched.size(), idx->e.size(),
            st.passes, st.a_batches, st.b_batches, C.batches, (unsigned long long)C.tiles, (unsigned long long)C.written,
            (unsigned long long)(st.h2d + C.h2d), (unsigned long long)(st.d2h + C.d2h));
  if (host) {
    CJS_TRY(C.room(1));                                                   // a buffer even for empty output
    *out = C.h_out; *out_n = (size_t)C.written;
    C.h_out = nullptr;
    return 0;
  }
  *out_need = (size_t)C.written;
  return C.written > C.cap ? (int)CJS_E_OUTPUT_TOO_SMALL : 0;
}

}  // namespace

extern "C" int cjs_bzip2_cut(const uint8_t* in, size_t n, const cjs_bz_index* idx, const cjs_bz_lines* lines, uint64_t first, uint64_t count, uint32_t mode,
                             uint32_t delim, const cjs_cut_range* sel, uint32_t nsel, uint8_t** out, size_t* out_n, cjs_bz_cut_info* info, const cjs_opts* opts) {
  CJS_GUARD_BEGIN
  if (!in && n) return CJS_E_INVALID_ARG;
  return cut_core(in ? in : (const uint8_t*)"", nullptr, n, idx, lines, first, count, mode, delim, sel, nsel, out, out_n, nullptr, 0, nullptr, info, opts);
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

extern "C" int cjs_bzip2_cut_device(const uint8_t* d_in, size_t n, const cjs_bz_index* idx, const cjs_bz_lines* lines, uint64_t first, uint64_t count, uint32_t mode,
                                    uint32_t delim, const cjs_cut_range* sel, uint32_t nsel, uint8_t* d_out, size_t out_cap, size_t* out_need,
                                    cjs_bz_cut_info* info, const cjs_opts* opts) {
  CJS_GUARD_BEGIN
  if (!d_in && n) return CJS_E_INVALID_ARG;
  return cut_core(nullptr, d_in, n, idx, lines, first, count, mode, delim, sel, nsel, nullptr, nullptr, d_out, out_cap, out_need, info, opts);
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

extern "C" int cjs_stage_cut(const uint8_t* text, size_t n, uint32_t mode, uint32_t delim, const cjs_cut_range* sel, uint32_t nsel, uint8_t* out, size_t cap,
                             size_t* out_n) {
  if ((!text && n) || (!out && cap) || !out_n) return CJS_E_INVALID_ARG;
  CtSel S;
  CJS_TRY(ct_normalise(mode, delim, sel, nsel, &S));
  *out_n = cut_text(S, text, n, out, cap);
  return *out_n > cap ? (int)CJS_E_OUTPUT_TOO_SMALL : 0;
}

extern "C" int cjs_cut_list_parse(const char* list, cjs_cut_range* sel, uint32_t cap, uint32_t* nsel) { return ct_parse_list(list, sel, cap, nsel); }
