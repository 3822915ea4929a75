// enc_index.hip -- the block rows of the compress pipeline: when a call has its blocks through the Huffman tables, every
// field of their index entries stands in device memory.  Two kernels gather them into 16-byte rows, one copy brings the rows down
// in front of the synchronisation the packing makes anyway, and the host (enc_index_plan.h) sets them at their bit offsets.
//   enc_rows     per block k of [f, f + cnt): bits = bitlen[k - f], crc = block_crc[k], size = blocks[k].e - blocks[k].s, newlines = 0
//   enc_newlines per 16 KiB tile of the input: the 0x0A bytes of the tile, added to the row of each block the tile lies in
// The three sources index differently: the Huffman buffers relative to f, the RLE1 tables from block 0 of the stream.
#include "ctx.h"
#include "range_engine.h"
#include "bz_lines.h"
#include "enc_index.h"
#include <memory>

using namespace cjs;

namespace cjs {

constexpr uint32_t ENC_NL_TILE = 16384;      // input bytes a workgroup counts: 256 lanes x 4 vectors of 16 bytes

__global__ __launch_bounds__(256) void enc_rows(const uint32_t* __restrict__ bitlen, const uint32_t* __restrict__ block_crc, const RleBlock* __restrict__ blocks,
                                                uint32_t f, uint32_t cnt, EncRow* __restrict__ rows) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= cnt) return;
  const RleBlock b = blocks[f + i];
  rows[i] = EncRow{bitlen[i], block_crc[f + i], (uint32_t)(b.e - b.s), 0u};
}

// Tile t is input bytes [16 Ki t, 16 Ki (t + 1)) below n.  The blocks [f, f + cnt) partition [blocks[f].s, blocks[f + cnt - 1].e):
// the tile's part of that span is cut at the block starts, each piece is counted as bounded aligned vectors (rg_span: nothing
// outside the piece is read, whatever the alignment of d_in) and added to its block's row.  A block of ~5 MB of runs collects
// hundreds of tiles in one word, a tile with a tiny last block gives to two rows or more.
__global__ __launch_bounds__(256) void enc_newlines(const uint8_t* __restrict__ d_in, uint64_t n, const RleBlock* __restrict__ blocks, uint32_t f, uint32_t cnt,
                                                    EncRow* __restrict__ rows) {
  __shared__ uint32_t sm[4];
  const uint64_t lo = max((uint64_t)blockIdx.x * ENC_NL_TILE, blocks[f].s);
  const uint64_t hi = min(min(((uint64_t)blockIdx.x + 1) * ENC_NL_TILE, n), blocks[f + cnt - 1].e);
  if (lo >= hi) return;                                   // (the same in every lane)
  uint32_t a = 0, b = cnt;                                // the last block of [f, f + cnt) that starts at or in front of lo
  while (b - a > 1) { const uint32_t mid = (a + b) >> 1; if (blocks[f + mid].s <= lo) a = mid; else b = mid; }
  for (uint32_t k = a; k < cnt; k++) {
    const RleBlock g = blocks[f + k];
    if (g.s >= hi) break;
    const uint64_t p0 = max(g.s, lo), p1 = min(g.e, hi);
    if (p0 >= p1) continue;
    const RgSpan S = rg_span((uint64_t)(uintptr_t)d_in + p0, (uint32_t)(p1 - p0));
    uint32_t c = 0;
    for (uint32_t v = threadIdx.x; v < S.nvec; v += 256) c += ln_count16(rg_vec(S, v));
    const uint32_t total = block_sum<256, uint32_t>(c, sm);
    if (threadIdx.x == 0 && total) atomicAdd(&rows[k].newlines, total);
  }
}

void enc_rows_destroy(EncRowsWork* w) { delete w; }

int enc_rows_enqueue(cjs_ctx* c, const uint8_t* d_in, size_t n, uint32_t f, uint32_t cnt, bool lines) {
  if (!cnt) return 0;
  if (cnt > c->range_blocks || (uint64_t)f + cnt > c->max_blocks) return CJS_E_INVALID_ARG;
  if (!c->enc_rows) c->enc_rows.reset(new EncRowsWork());
  EncRowsWork& w = *c->enc_rows.p;
  if (w.cap < c->range_blocks) {                          // the context's first indexed call
    w.cap = 0;
    CJS_TRY(w.d.alloc(sizeof(EncRow) * c->range_blocks));
    CJS_HIP_TRY(hipHostMalloc((void**)w.h.put(), sizeof(EncRow) * c->range_blocks));
    w.cap = c->range_blocks;
  }
  hipStream_t s = c->stream;
  hipLaunchKernelGGL(enc_rows, dim3((cnt + 255) / 256), dim3(256), 0, s, (const uint32_t*)c->huff.b.bitlen, (const uint32_t*)c->rle.block_crc,
                     (const RleBlock*)c->rle.blocks, f, cnt, w.d.p);
  const uint64_t tiles = ((uint64_t)n + ENC_NL_TILE - 1) / ENC_NL_TILE;
  if (lines && tiles) {
    if (tiles > 0x7FFFFFFFull) return CJS_E_UNSUPPORTED;
    hipLaunchKernelGGL(enc_newlines, dim3((unsigned)tiles), dim3(256), 0, s, d_in, (uint64_t)n, (const RleBlock*)c->rle.blocks, f, cnt, w.d.p);
  }
  CJS_HIP_TRY(hipGetLastError());
  CJS_HIP_TRY(hipMemcpyAsync(w.h.p, w.d.p, sizeof(EncRow) * cnt, hipMemcpyDeviceToHost, s));
  return 0;
}

void enc_rows_collect(const cjs_ctx* c, uint32_t cnt, EncRowsWant& want) {
  if (cnt) want.rows.insert(want.rows.end(), c->enc_rows.p->h.p, c->enc_rows.p->h.p + cnt);
}

int enc_tables_make(const std::vector<cjs_bz_index_entry>& entries, const std::vector<uint32_t>& newlines, uint64_t end_bit, cjs_bz_index** idx,
                    cjs_bz_lines** lines) {
  *idx = nullptr;
  if (lines) *lines = nullptr;
  cjs_bz_index* made = nullptr;
  if (bz_index_make(entries.data(), entries.size(), enc_stream_bytes(end_bit), false, &made)) return CJS_E_HIP;
  std::unique_ptr<cjs_bz_index> ix(made);
  if (lines && bz_lines_make(made, newlines.data(), newlines.size(), lines)) return CJS_E_HIP;
  *idx = ix.release();
  return 0;
}

}  // namespace cjs
