// huff_pack.hip — bzip2 entropy stage on the GPU, the packer: bit offsets of the blocks, the blocks' headers, selectors and tables
// (pack_block), their symbol data (pack_data), the stream frame, and the same for batches of independent streams.
//
// Replaces J/Bzip2_joined_.js: selector unary :2167-2182, StaticHuffman.emit/encode :1926-1951, data loop :2189-2194,
// BitStream.writeBits :154-166.  What an item is and how long is huff_rules.h (the accounting of huff_tables.hip adds the same
// items' lengths).  Bit packing: wave prefix-scan of code lengths -> bit offsets -> words assembled in LDS -> coalesced
// big-endian stores.
#include "cjs_internal.h"
#include "prims.hpp"
#include "huff.h"

namespace cjs {

// ------------------------------------------------------------------ bit offsets + stream CRC (one lane, tiny)
// also the output size check (no host round trip for it): too_small[0] = 1 stops the pack kernels before they write anything
__global__ void huff_offsets(HuffBufs hb, const uint32_t* __restrict__ block_crc, uint32_t nb, uint32_t first, uint32_t count,
                             uint64_t start_bit, uint32_t* __restrict__ stream_crc_out, uint64_t trailer_bits, uint64_t cap_bytes,
                             uint64_t* __restrict__ too_small, int crc_given, uint32_t crc_value) {
  if (threadIdx.x || blockIdx.x) return;
  (void)first;
  uint64_t bit = start_bit;                         // per-block buffers are indexed relative to `first`
  for (uint32_t k = 0; k < count; k++) { hb.bitoff[k] = bit; bit += hb.bitlen[k]; }
  hb.bitoff[count] = bit;
  too_small[0] = stream_too_small(bit, trailer_bits, cap_bytes) ? 1u : 0u;
  uint32_t c = crc_value;                           // (a rank of a multi-GPU job is handed the fold over all ranks' blocks)
  if (!crc_given) { c = 0; for (uint32_t k = 0; k < nb; k++) c = ((c << 1) | (c >> 31)) ^ block_crc[k]; }      // Bzip2:2237
  *stream_crc_out = c;
}

// zeroes the part of the output the stream will occupy (the pack kernels OR their boundary words into it): the stream end is
// known on the device (bitoff[count]); the rest of the caller's buffer is left as it is
__global__ __launch_bounds__(256) void pack_zero_output(HuffBufs hb, uint32_t count, uint64_t trailer_bits, uint32_t* __restrict__ out32, uint64_t cap_bytes,
                                                        const uint64_t* __restrict__ too_small) {
  if (too_small[0]) return;
  const uint64_t nw = stream_zeroed_bytes(hb.bitoff[count], trailer_bits, cap_bytes) / 4;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < nw; i += (uint64_t)gridDim.x * 256) out32[i] = 0;
}

// ------------------------------------------------------------------ bit packing
// Put `nbits` (<= 64) of `val` at absolute stream bit `bit` into LDS words indexed from word0.
__device__ __forceinline__ void put_bits(uint32_t* words, uint64_t word0, uint64_t bit, uint64_t val, uint32_t nbits) {
  split_bits(bit, val, nbits, [&](uint64_t w, uint32_t piece) { atomicOr(&words[w - word0], piece); });
}

constexpr int PK_ITEMS = 4;                       // items per thread per tile
constexpr int PK_WORDS = (1024 * PK_ITEMS * 40) / 32 + 8;

template <typename F>
__device__ void pack_phase(uint32_t count, F item_fn, uint32_t* words, uint32_t* sm, uint64_t& bit, uint32_t* __restrict__ out32) {
  for (uint32_t base = 0; base < count; base += 1024 * PK_ITEMS) {
    BitItem it[PK_ITEMS];
    uint32_t nb = 0;
#pragma unroll
    for (int j = 0; j < PK_ITEMS; j++) {
      const uint32_t i = base + threadIdx.x * PK_ITEMS + j;
      it[j].val = 0; it[j].nbits = 0;
      if (i < count) it[j] = item_fn(i);
      nb += it[j].nbits;
    }
    uint32_t tot;
    const uint32_t ex = block_excl_sum<1024>(nb, sm, tot);
    const uint64_t word0 = bit >> 5;
    const uint32_t nwords = (uint32_t)(((bit + tot + 31) >> 5) - word0);
    for (uint32_t i = threadIdx.x; i < nwords; i += 1024) words[i] = 0;
    __syncthreads();
    uint64_t b = bit + ex;
    {                                                   // the thread's items as one or two strings of <= 64 bits: fewer LDS atomics on shared words
      uint64_t pv = 0; uint32_t pn = 0;
#pragma unroll
      for (int j = 0; j < PK_ITEMS; j++) {
        if (pn + it[j].nbits > 64u) { put_bits(words, word0, b, pv, pn); b += pn; pv = 0; pn = 0; }
        pv = it[j].nbits >= 64u ? it[j].val : ((pv << it[j].nbits) | (it[j].val & ((1ull << it[j].nbits) - 1ull)));
        pn += it[j].nbits;
      }
      put_bits(words, word0, b, pv, pn);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < nwords; i += 1024) {
      const uint32_t v = __builtin_bswap32(words[i]);
      if (i == 0 || i == nwords - 1) { if (v) atomicOr(&out32[word0 + i], v); }
      else out32[word0 + i] = v;
    }
    __syncthreads();
    bit += tot;
  }
}

__global__ __launch_bounds__(1024) void pack_block(HuffBufs hb, uint32_t first, const uint16_t* __restrict__ Aall, size_t a_stride,
                                                   const uint32_t* __restrict__ npos_all, const uint32_t* __restrict__ asz_all,
                                                   const uint8_t* __restrict__ alist_all, const uint32_t* __restrict__ block_crc,
                                                   const uint32_t* __restrict__ pidx_all, uint32_t* __restrict__ out32,
                                                   const uint64_t* __restrict__ too_small) {
  __shared__ uint32_t words[PK_WORDS];
  __shared__ uint32_t sm[16];
  __shared__ uint32_t used16[17];
  if (too_small[0]) return;
  __shared__ uint32_t ctab[MAXTAB * MAXSYM];
  __shared__ uint8_t ltab[MAXTAB * MAXSYM + 4];
  const uint32_t blk = blockIdx.x;                  // relative to `first`; block_crc is absolute
  const uint32_t npos = npos_all[blk], asz = asz_all[blk], ng = hb.ngroups[blk];
  const uint32_t n = asz + 2, nsel = groups_for(npos);
  (void)Aall; (void)a_stride;
  const uint8_t* selj = hb.selj + (size_t)blk * hb.sel_stride;
  for (uint32_t i = threadIdx.x; i < MAXTAB * MAXSYM; i += 1024) { ctab[i] = hb.codes[(size_t)blk * MAXTAB * MAXSYM + i]; ltab[i] = hb.lens[(size_t)blk * MAXTAB * MAXSYM + i]; }
  if (threadIdx.x < 17) used16[threadIdx.x] = 0;
  __syncthreads();
  if (threadIdx.x < asz) {
    const uint32_t v = alist_all[(size_t)blk * 256 + threadIdx.x];
    atomicOr(&used16[1 + (v >> 4)], 0x8000u >> (v & 15));
    atomicOr(&used16[0], 0x8000u >> (v >> 4));
  }
  __syncthreads();
  uint64_t bit = hb.bitoff[blk];
  const uint32_t crc = block_crc[first + blk], pidx = pidx_all[blk];
  const uint32_t coarse = used16[0];
  pack_phase(HEADER_ITEMS, [&](uint32_t i) -> BitItem { return header_item(i, crc, pidx, coarse, used16 + 1, ng, nsel); }, words, sm, bit, out32);
  // selectors, MTF + unary (Bzip2:2171-2182)
  pack_phase(nsel, [&](uint32_t g) -> BitItem { return selector_item(selj[g]); }, words, sm, bit, out32);
  // tables (Bzip2:1926-1947)
  pack_phase(ng * n, [&](uint32_t i) -> BitItem {
    const uint32_t t = i / n, s = i - t * n;
    const uint32_t cur = ltab[t * MAXSYM + s], prev = s ? ltab[t * MAXSYM + s - 1] : cur;
    return table_item(cur, prev, s == 0);
  }, words, sm, bit, out32);
  // the symbol data follows: pack_data, one workgroup per 4000-symbol tile
}

// data (Bzip2:2189-2194): tile `blockIdx.x` of block `blockIdx.y`; its first bit = block start + block bits - data bits +
// the tile's offset from huff_block.  Interior words are plain stores, the two boundary words are OR-ed.
__global__ __launch_bounds__(1024) void pack_data(HuffBufs hb, const uint16_t* __restrict__ Aall, size_t a_stride, const uint32_t* __restrict__ npos_all,
                                                  uint32_t* __restrict__ out32, const uint64_t* __restrict__ too_small) {
  __shared__ uint32_t words[PK_WORDS];
  __shared__ uint32_t sm[16];
  __shared__ uint32_t ctab[MAXTAB * MAXSYM];
  __shared__ uint8_t ltab[MAXTAB * MAXSYM + 4];
  if (too_small[0]) return;
  const uint32_t blk = blockIdx.y, tile = blockIdx.x;
  const uint32_t npos = npos_all[blk], nsel = groups_for(npos);
  if (tile * PD_GROUPS >= nsel) return;
  const uint16_t* A = Aall + (size_t)blk * a_stride;
  const uint8_t* sel = hb.sel + (size_t)blk * hb.sel_stride;
  for (uint32_t i = threadIdx.x; i < MAXTAB * MAXSYM; i += 1024) { ctab[i] = hb.codes[(size_t)blk * MAXTAB * MAXSYM + i]; ltab[i] = hb.lens[(size_t)blk * MAXTAB * MAXSYM + i]; }
  __syncthreads();
  uint64_t bit = hb.bitoff[blk] + hb.bitlen[blk] - hb.databits[blk] + hb.tileoff[(size_t)blk * hb.tile_stride + tile];
  const uint32_t i0 = tile * PD_GROUPS * GSZ;
  const uint32_t cnt = npos - i0 < (uint32_t)(PD_GROUPS * GSZ) ? npos - i0 : (uint32_t)(PD_GROUPS * GSZ);
  pack_phase(cnt, [&](uint32_t i) -> BitItem {
    const uint32_t t = sel[(i0 + i) / GSZ], s = A[i0 + i];
    return BitItem{ctab[t * MAXSYM + s], ltab[t * MAXSYM + s]};
  }, words, sm, bit, out32);
}

// stream header / trailer.  One lane.
// follow_magic: the blocks of the next rank of a multi-GPU job follow this fragment: the last word of the fragment is completed
// with the leading bits of what comes next in the stream -- always the 48-bit block magic -- so that the ranks' fragments are
// disjoint runs of whole 32-bit words of the one stream (the next rank leaves its first, partial word out of its fragment).
__global__ void pack_frame(HuffBufs hb, uint32_t nb_range_end, int level, int write_header, int write_trailer, int follow_magic,
                           const uint32_t* __restrict__ stream_crc, uint32_t* __restrict__ out32, uint64_t* __restrict__ total_bits) {
  if (threadIdx.x || blockIdx.x) return;
  if (total_bits[2]) { total_bits[0] = hb.bitoff[nb_range_end] + (write_trailer ? STREAM_TRAILER_BITS : 0u); return; }      // output too small: nothing is written
  if (write_header) atomicOr(&out32[0], __builtin_bswap32(BZH0_WORD + (uint32_t)level));   // 'B''Z''h''0'+level
  uint64_t bit = hb.bitoff[nb_range_end];
  if (follow_magic && !write_trailer && (bit & 31)) {
    const uint32_t room = 32 - (uint32_t)(bit & 31);
    atomicOr(&out32[bit >> 5], __builtin_bswap32((uint32_t)(MAGIC_BLOCK >> (48 - room))));
  }
  if (write_trailer) bit = put_trailer_words(out32, bit, *stream_crc);
  *total_bits = bit;
}

// ------------------------------------------------------------------ batches of independent streams
// framed: stream j = 'BZh<level>', block j, end-of-stream magic and CRC (= the block's CRC: the fold of one block from 0);
// else the bare bit string of block j from bit 0 (a block of an input of several blocks, assembled into its stream later).
// They follow each other at 4-byte-aligned byte offsets from `base`; one workgroup scans their sizes.  sc[0] = total bytes
// (aligned), sc[2] = 0 (the pack kernels' "output too small" flag: the caller has made room).
__global__ __launch_bounds__(1024) void huff_batch_offsets(HuffBufs hb, uint32_t nb, uint64_t base, int framed, uint64_t* __restrict__ soff,
                                                          uint32_t* __restrict__ slen, uint64_t* __restrict__ sc) {
  __shared__ uint64_t sm[16];
  uint64_t run = 0;
  for (uint32_t c0 = 0; c0 < nb; c0 += 1024) {
    const uint32_t j = c0 + threadIdx.x;
    const uint64_t bytes = j < nb ? ((framed ? framed_bits(hb.bitlen[j]) : (uint64_t)hb.bitlen[j]) + 7u) / 8u : 0u;
    uint64_t tot;
    const uint64_t ex = block_excl_sum<1024>((bytes + 3u) & ~(uint64_t)3, sm, tot);
    if (j < nb) { const uint64_t o = base + run + ex; soff[j] = o; slen[j] = (uint32_t)bytes; hb.bitoff[j] = o * 8u + (framed ? STREAM_HEADER_BITS : 0u); }
    run += tot;
  }
  if (threadIdx.x == 0) { sc[0] = run; sc[2] = 0; }
}
// header word and trailer of every stream (the pack kernels have written the block behind the header word)
__global__ __launch_bounds__(256) void huff_batch_frame(HuffBufs hb, uint32_t nb, int level, const uint32_t* __restrict__ block_crc,
                                                        const uint64_t* __restrict__ soff, uint32_t* __restrict__ out32) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= nb) return;
  out32[soff[j] >> 2] = __builtin_bswap32(BZH0_WORD + (uint32_t)level);      // 'B''Z''h''0'+level (a word of its own)
  put_trailer_words(out32, hb.bitoff[j] + hb.bitlen[j], block_crc[j]);
}

int huff_batch_offsets_run(hipStream_t s, HuffWork& w, uint32_t nb, uint64_t base, int framed, uint64_t* d_soff, uint32_t* d_slen) {
  if (!nb) return 0;
  hipLaunchKernelGGL(huff_batch_offsets, dim3(1), dim3(1024), 0, s, w.b, nb, base, framed, d_soff, d_slen, w.scalars);
  CJS_HIP_TRY(hipGetLastError());
  return 0;
}
int huff_batch_pack_run(hipStream_t s, HuffWork& w, const SymRows& r, const PackJob& j, const uint64_t* d_soff) {
  const uint32_t nb = j.count;
  if (!nb) return 0;
  hipLaunchKernelGGL(pack_block, dim3(nb), dim3(1024), 0, s, w.b, 0u, r.A, r.a_stride, r.npos, r.asz, r.alist, j.block_crc, j.pidx, j.out32, w.scalars + 2);
  hipLaunchKernelGGL(pack_data, dim3((unsigned)(w.b.tile_stride - 1), nb), dim3(1024), 0, s, w.b, r.A, r.a_stride, r.npos, j.out32, w.scalars + 2);
  if (j.header) hipLaunchKernelGGL(huff_batch_frame, dim3((nb + 255) / 256), dim3(256), 0, s, w.b, nb, j.level, j.block_crc, d_soff, j.out32);
  CJS_HIP_TRY(hipGetLastError());
  return 0;
}

int huff_pack_run(hipStream_t s, HuffWork& w, const SymRows& r, const PackJob& j) {
  uint32_t* stream_crc = (uint32_t*)(w.scalars + 1);
  const PackShard* ps = j.shard;
  const uint64_t trailer_bits = j.trailer ? STREAM_TRAILER_BITS : 0;
  hipLaunchKernelGGL(huff_offsets, dim3(1), dim3(1), 0, s, w.b, j.block_crc, j.nb_total, j.first, j.count, j.start_bit, stream_crc,
                     trailer_bits, (uint64_t)j.out_cap_bytes, w.scalars + 2, ps ? 1 : 0, ps ? ps->stream_crc : 0u);
  hipLaunchKernelGGL(pack_zero_output, dim3(4096), dim3(256), 0, s, w.b, j.count, trailer_bits, j.out32, (uint64_t)j.out_cap_bytes, w.scalars + 2);
  if (j.count) {
    hipLaunchKernelGGL(pack_block, dim3(j.count), dim3(1024), 0, s, w.b, j.first, r.A, r.a_stride, r.npos, r.asz, r.alist, j.block_crc, j.pidx, j.out32, w.scalars + 2);
    hipLaunchKernelGGL(pack_data, dim3((unsigned)(w.b.tile_stride - 1), j.count), dim3(1024), 0, s, w.b, r.A, r.a_stride, r.npos, j.out32, w.scalars + 2);
  }
  hipLaunchKernelGGL(pack_frame, dim3(1), dim3(1), 0, s, w.b, j.count, j.level, j.header ? 1 : 0, j.trailer ? 1 : 0, ps ? ps->follow_magic : 0, stream_crc, j.out32, w.scalars);
  CJS_HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace cjs
