// batch.hip — Bzip2.compressFile over a batch of independent inputs (cjs_bzip2_compress_batch*): one .bz2 stream per input,
// stream k byte-identical to cjs_bzip2_compress(input k).  Every stage runs over whole passes of blocks, not once per input:
//   RLE1 length of every input (one workgroup per input)                     -> host: one block / several blocks / empty
//   block boundaries of the inputs of several blocks (one workgroup per input)
//   passes over the blocks (one-block inputs, and the blocks of the other inputs, each list by descending length):
//     RLE1 bytes (one workgroup per block) + CRC of every block (crc_ranges)
//     suffix sort over blocks of different lengths (bwt_run_var) -> MTF / RLE2 -> Huffman tables (per-block lengths already)
//     offsets (one-workgroup scan) -> one-block inputs: header + block + trailer at their own 4-byte-aligned offset;
//                                     blocks of the other inputs: bare bit strings
//   the streams of the inputs of several blocks: every block's bit string shifted to its place (one workgroup per block),
//     header and trailer with the stream CRC folded over the input's blocks
//   empty inputs: the 14-byte empty stream
// The streams are assembled in a staging buffer of the context; they reach the caller's buffer only once every size is known.
#include "crc.h"
#include "ctx.h"
#include "host.h"
#include "prims.hpp"
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>

using namespace cjs;

namespace cjs {

constexpr uint32_t BATCH_MAX_ITEMS = 65535;          // blocks of a sub-batch (grid y of the per-block kernels)
constexpr size_t BATCH_MAX_ELEMS = (size_t)1 << 29;   // slots of a sub-batch (suffix-sort workspace ~50 B each)
constexpr uint32_t SMALL_SLOT = 512;                  // slots up to this wide: every block of the list shares the pass

struct BatchWork {
  Arena arena;                     // re-carved for every sub-batch
  size_t elems = 0;                // slot budget the arena was sized for
  uint32_t items = 0;              // blocks per sub-batch
  BwtWork bwt;
  MtfWork mtf;
  HuffWork huff;
  DevMem<uint8_t> stage;           // the streams of a call, back to back
  size_t stage_cap = 0;
  DevMem<uint8_t> scratch;         // bare bit strings of the blocks of inputs of several blocks, before they are assembled
  size_t scratch_cap = 0;
  Pinned<uint64_t> h_sc;           // scalars
};

void batch_destroy(BatchWork* b) { delete b; }

namespace {

// a block of the batch: RLE1 of in[s, e) (relative to the call's d_in), len bytes; input number and block number in that input
struct BItem { uint64_t s, e; uint32_t len, input, blk; };

// bytes of the sub-batch workspace for nb blocks in slots of `stride`, CRC windows `segs` per block
size_t sub_bytes(size_t nb, uint32_t stride, size_t segs) {
  const size_t e = nb * stride;
  return BwtWork::bytes_needed(e) + MtfWork::bytes_needed(nb, stride) + HuffWork::bytes_needed(nb, stride) +
         2 * (e + 256) + nb * (4 * 5 + 8 + sizeof(RleBlock) + 4 * segs) + 24 * 256 + 4096;
}

// the empty stream: 'BZh<level>', end-of-stream magic, CRC 0 (14 bytes; the slot is 16)
__global__ __launch_bounds__(256) void batch_empty_streams(const uint64_t* __restrict__ off, uint32_t n, int level, uint32_t* __restrict__ out32) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  uint32_t* o = out32 + (off[i] >> 2);
  o[0] = __builtin_bswap32(BZH0_WORD + (uint32_t)level);
  o[1] = __builtin_bswap32(0x17724538u);
  o[2] = __builtin_bswap32(0x50900000u);
  o[3] = 0;
}

// Streams of inputs of several blocks: block j's bare bit string (src, 4-byte aligned, nbits) goes to stream bit dst_bit of out
// (zeroed; every word OR-ed: a word may be shared with the block in front).  One workgroup per block.
struct AsmBlock { uint64_t src, dst_bit; uint64_t nbits; };
__global__ __launch_bounds__(256) void batch_asm_blocks(const AsmBlock* __restrict__ tab, const uint32_t* __restrict__ src32, uint32_t* __restrict__ out32) {
  const AsmBlock t = tab[blockIdx.x];
  if (!t.nbits) return;
  const uint32_t* sw = src32 + (t.src >> 2);
  const uint64_t nsw = (t.nbits + 31) >> 5;
  const uint32_t r = (uint32_t)(t.dst_bit & 31);
  const uint64_t dw0 = t.dst_bit >> 5, ndw = ((t.dst_bit + t.nbits - 1) >> 5) - dw0 + 1;
  for (uint64_t i = threadIdx.x; i < ndw; i += 256) {
    const uint32_t cur = i < nsw ? __builtin_bswap32(sw[i]) : 0u;
    const uint32_t prev = i && i - 1 < nsw ? __builtin_bswap32(sw[i - 1]) : 0u;
    const uint32_t v = r ? (prev << (32 - r)) | (cur >> r) : cur;
    if (v) atomicOr(&out32[dw0 + i], __builtin_bswap32(v));
  }
}
// header word and trailer (end-of-stream magic, stream CRC at end_bit) of those streams
struct AsmStream { uint64_t off, end_bit; uint32_t crc, pad; };
__global__ __launch_bounds__(256) void batch_asm_frame(const AsmStream* __restrict__ tab, uint32_t n, int level, uint32_t* __restrict__ out32) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const AsmStream t = tab[i];
  atomicOr(&out32[t.off >> 2], __builtin_bswap32(BZH0_WORD + (uint32_t)level));
  put_trailer_words(out32, t.end_bit, t.crc);
}

// One sub-batch: blocks it[0..nb) in slots of `stride`, through every stage in one pass.  framed: every block is a stream of its
// own (into the staging buffer), else a bare bit string (into the scratch buffer), both from byte `base` on.  res[at + j]: block j.
struct BlockOuts {                   // per block: byte offset, byte length, bit length, CRC
  std::vector<uint64_t> so;
  std::vector<uint32_t> sl, bits, crc;
  void resize(size_t n) { so.resize(n); sl.resize(n); bits.resize(n); crc.resize(n); }
};
int run_sub(cjs_ctx* c, const uint8_t* d_in, const BItem* it, uint32_t nb, uint32_t stride, size_t segs, int level, bool framed, uint64_t base,
            BlockOuts& res, size_t at, uint64_t* bytes) {
  BatchWork& b = *c->batch;
  hipStream_t s = c->stream;
  Arena& a = b.arena;
  a.used = 0;
  const size_t e = (size_t)nb * stride;
  CJS_TRY(b.bwt.carve(a, e));
  CJS_TRY(b.mtf.carve(a, nb, stride));
  CJS_TRY(b.huff.carve(a, nb, stride));
  uint8_t* d_blocks = a.take<uint8_t>(e + 16);
  uint8_t* d_U = a.take<uint8_t>(e + 16);
  uint32_t* d_pidx = a.take<uint32_t>(nb);
  uint32_t* d_blen = a.take<uint32_t>(nb);
  uint32_t* d_crc = a.take<uint32_t>(nb);
  uint32_t* d_slen = a.take<uint32_t>(nb);
  uint32_t* d_nb = a.take<uint32_t>(16);
  uint64_t* d_soff = a.take<uint64_t>(nb);
  RleBlock* d_rb = a.take<RleBlock>(nb);
  uint32_t* d_seg = a.take<uint32_t>((size_t)nb * segs);
  if (!d_seg) return CJS_E_OUT_OF_MEMORY;                 // (sub_bytes() is what the caller checked: cannot happen)
  std::vector<RleBlock> rb(nb);
  std::vector<uint32_t> rl(nb);
  for (uint32_t j = 0; j < nb; j++) { rb[j] = RleBlock{}; rb[j].s = it[j].s; rb[j].e = it[j].e; rb[j].len = rl[j] = it[j].len; }
  const uint32_t nbv = nb;
  CJS_HIP_TRY(hipMemcpyAsync(d_blen, rl.data(), 4 * (size_t)nb, hipMemcpyHostToDevice, s));
  CJS_HIP_TRY(hipMemcpyAsync(d_rb, rb.data(), sizeof(RleBlock) * nb, hipMemcpyHostToDevice, s));
  CJS_HIP_TRY(hipMemcpyAsync(d_nb, &nbv, 4, hipMemcpyHostToDevice, s));
  CJS_TRY(rle1_batch_materialize(s, d_in, d_rb, nb, stride, d_blocks));
  CJS_TRY(crc_ranges(s, d_in, d_rb, d_nb, nb, (uint32_t)segs, d_seg, d_crc));
  CJS_TRY(bwt_run_var(s, b.bwt, d_blocks, nb, stride, d_blen, d_U, d_pidx));
  CJS_TRY(mtf_run(s, b.mtf, d_U, nb, d_blen));
  CJS_TRY(huff_tables_run(s, b.huff, nb, b.mtf.rows()));
  CJS_TRY(huff_batch_offsets_run(s, b.huff, nb, base, framed ? 1 : 0, d_soff, d_slen));
  CJS_HIP_TRY(hipMemcpyAsync(b.h_sc, b.huff.scalars, 8, hipMemcpyDeviceToHost, s));
  CJS_HIP_TRY(hipStreamSynchronize(s));                  // (the output buffer may have to grow before the streams are written)
  const uint64_t total = b.h_sc[0];
  DevMem<uint8_t>& buf = framed ? b.stage : b.scratch;
  size_t& cap = framed ? b.stage_cap : b.scratch_cap;
  CJS_TRY(DevCache::grow(buf, cap, base + total + 16, true, s));
  CJS_HIP_TRY(hipMemsetAsync(buf + base, 0, total + 16, s));
  PackJob job{nb, 0, nb, 0, level, framed, framed, d_crc, d_pidx, (uint32_t*)buf.p, 0};
  CJS_TRY(huff_batch_pack_run(s, b.huff, b.mtf.rows(), job, d_soff));
  CJS_HIP_TRY(hipMemcpyAsync(res.so.data() + at, d_soff, 8 * (size_t)nb, hipMemcpyDeviceToHost, s));
  CJS_HIP_TRY(hipMemcpyAsync(res.sl.data() + at, d_slen, 4 * (size_t)nb, hipMemcpyDeviceToHost, s));
  CJS_HIP_TRY(hipMemcpyAsync(res.bits.data() + at, b.huff.b.bitlen, 4 * (size_t)nb, hipMemcpyDeviceToHost, s));
  CJS_HIP_TRY(hipMemcpyAsync(res.crc.data() + at, d_crc, 4 * (size_t)nb, hipMemcpyDeviceToHost, s));
  CJS_HIP_TRY(hipStreamSynchronize(s));
  *bytes = total;
  return 0;
}

// Runs of a list of blocks sorted by descending length through run_sub.  A run ends where the workspace (or 65535 blocks) is
// full, or, for slots wider than SMALL_SLOT, where a block is shorter than half the run's first one (bounds the slots left empty
// behind the shorter blocks; narrow slots cost little, so tiny inputs all share one pass).
int run_list(cjs_ctx* c, const uint8_t* d_in, const std::vector<BItem>& L, int level, bool framed, uint64_t& used, uint32_t& passes, BlockOuts& res) {
  BatchWork& b = *c->batch;
  res.resize(L.size());
  for (size_t i0 = 0; i0 < L.size();) {
    const uint32_t stride = (L[i0].len + 15u) & ~15u;
    size_t segs = 0, i1 = i0;
    while (i1 < L.size() && i1 - i0 < b.items && (i1 == i0 || stride <= SMALL_SLOT || (size_t)L[i1].len * 2 >= L[i0].len)) {
      const size_t sg = std::max<size_t>(segs, (L[i1].e - L[i1].s) / 16384 + 2);
      const size_t nb = i1 - i0 + 1;
      if (nb > 1 && (sub_bytes(nb, stride, sg) > b.arena.cap || nb * stride >= 0xFFFFF000ull)) break;
      segs = sg; i1++;
    }
    if (sub_bytes(i1 - i0, stride, segs) > b.arena.cap) return CJS_E_OUT_OF_MEMORY;     // the workspace cannot take even one block
    uint64_t bytes = 0;
    CJS_TRY(run_sub(c, d_in, L.data() + i0, (uint32_t)(i1 - i0), stride, segs, level, framed, used, res, i0, &bytes));
    used += bytes;
    passes++;
    i0 = i1;
  }
  return 0;
}

}  // namespace

// The streams of inputs d_in[st[k] .. en[k]) (k < count) into the context's staging buffer; out_off / out_len per input,
// *end = end of the last stream in the staging buffer.
static int batch_core(cjs_ctx* c, const uint8_t* d_in, const std::vector<uint64_t>& st, const std::vector<uint64_t>& en, size_t count,
                      int level, size_t* out_off, size_t* out_len, uint64_t* end) {
  BatchWork& b = *c->batch;
  hipStream_t s = c->stream;
  *end = 0;
  std::vector<uint64_t> se(2 * count);
  for (size_t k = 0; k < count; k++) { se[2 * k] = st[k]; se[2 * k + 1] = en[k]; }
  // RLE1 length of every input
  DevBuf se_buf(16 * count + 8 * count);
  uint64_t* d_se = (uint64_t*)se_buf.p;
  if (!d_se) return CJS_E_OUT_OF_MEMORY;
  uint64_t* d_len2 = d_se + 2 * count;
  CJS_HIP_TRY(hipMemcpyAsync(d_se, se.data(), 16 * count, hipMemcpyHostToDevice, s));
  CJS_TRY(rle1_batch_len(s, d_in, d_se, (uint32_t)count, c->cap, d_len2));
  std::vector<uint64_t> len2(count);
  CJS_HIP_TRY(hipMemcpyAsync(len2.data(), d_len2, 8 * count, hipMemcpyDeviceToHost, s));
  CJS_HIP_TRY(hipStreamSynchronize(s));
  std::vector<BItem> one, parts;
  std::vector<uint32_t> multi, empty;
  for (size_t k = 0; k < count; k++) {
    const uint64_t L = len2[k] >> 1;
    if (en[k] == st[k]) empty.push_back((uint32_t)k);
    else if (L < c->cap || (L == c->cap && !(len2[k] & 1))) one.push_back(BItem{st[k], en[k], (uint32_t)L, (uint32_t)k, 0});
    else multi.push_back((uint32_t)k);
  }
  // block boundaries of the inputs of several blocks: one workgroup per input
  if (!multi.empty()) {
    std::vector<uint32_t> tbase(multi.size() + 1, 0);
    for (size_t j = 0; j < multi.size(); j++) tbase[j + 1] = tbase[j] + (uint32_t)Rle1Work::max_blocks_for(en[multi[j]] - st[multi[j]], c->cap);
    const size_t nt = tbase.back();
    DevBuf wb(4 * multi.size() + 4 * (multi.size() + 1) + 4 * multi.size() + sizeof(RleBlock) * nt + 64);
    uint8_t* w = (uint8_t*)wb.p;
    if (!w) return CJS_E_OUT_OF_MEMORY;
    RleBlock* d_tab = (RleBlock*)w;
    uint32_t* d_item = (uint32_t*)(w + sizeof(RleBlock) * nt);
    uint32_t* d_tbase = d_item + multi.size();
    uint32_t* d_nblk = d_tbase + multi.size() + 1;
    CJS_HIP_TRY(hipMemcpyAsync(d_item, multi.data(), 4 * multi.size(), hipMemcpyHostToDevice, s));
    CJS_HIP_TRY(hipMemcpyAsync(d_tbase, tbase.data(), 4 * tbase.size(), hipMemcpyHostToDevice, s));
    CJS_TRY(rle1_batch_walk(s, d_in, d_se, d_item, d_tbase, (uint32_t)multi.size(), c->cap, d_tab, d_nblk));
    std::vector<RleBlock> tab(nt);
    std::vector<uint32_t> nblk(multi.size());
    CJS_HIP_TRY(hipMemcpyAsync(tab.data(), d_tab, sizeof(RleBlock) * nt, hipMemcpyDeviceToHost, s));
    CJS_HIP_TRY(hipMemcpyAsync(nblk.data(), d_nblk, 4 * multi.size(), hipMemcpyDeviceToHost, s));
    CJS_HIP_TRY(hipStreamSynchronize(s));
    for (size_t j = 0; j < multi.size(); j++) {
      if (nblk[j] > tbase[j + 1] - tbase[j]) return CJS_E_HIP;     // cannot happen: a full block takes at least 4/5 of cap bytes
      const uint32_t k = multi[j];
      for (uint32_t q = 0; q < nblk[j]; q++) {
        const RleBlock& r = tab[tbase[j] + q];
        parts.push_back(BItem{st[k] + r.s, st[k] + r.e, r.len, k, q});
      }
    }
  }
  auto by_len = [](const BItem& x, const BItem& y) { return x.len > y.len; };
  std::stable_sort(one.begin(), one.end(), by_len);
  std::stable_sort(parts.begin(), parts.end(), by_len);
  uint64_t used = 0, sused = 0;
  uint32_t passes = 0;
  BlockOuts r;
  CJS_TRY(run_list(c, d_in, one, level, true, used, passes, r));
  for (size_t i = 0; i < one.size(); i++) { out_off[one[i].input] = (size_t)r.so[i]; out_len[one[i].input] = r.sl[i]; }
  // inputs of several blocks: their blocks' bit strings (scratch), then assembled into streams behind the others
  if (!parts.empty()) {
    CJS_TRY(run_list(c, d_in, parts, level, false, sused, passes, r));
    std::vector<size_t> at(multi.size() + 1, 0), pos(count, 0);
    for (size_t j = 0; j < multi.size(); j++) pos[multi[j]] = j;
    std::vector<size_t> cnt(multi.size(), 0);
    for (const BItem& x : parts) cnt[pos[x.input]]++;
    for (size_t j = 0; j < multi.size(); j++) at[j + 1] = at[j] + cnt[j];
    std::vector<size_t> order(parts.size());                 // parts index of block q of multi input j: order[at[j] + q]
    for (size_t i = 0; i < parts.size(); i++) order[at[pos[parts[i].input]] + parts[i].blk] = i;
    std::vector<AsmBlock> ab(parts.size());
    std::vector<AsmStream> as(multi.size());
    const uint64_t used0 = used;
    for (size_t j = 0; j < multi.size(); j++) {
      uint64_t bit = used * 8 + 32;
      uint32_t scrc = 0;
      for (size_t q = 0; q < cnt[j]; q++) {
        const size_t i = order[at[j] + q];
        ab[at[j] + q] = AsmBlock{r.so[i], bit, r.bits[i]};
        bit += r.bits[i];
        scrc = crc_fold(scrc, r.crc[i]);
      }
      as[j] = AsmStream{used, bit, scrc, 0};
      out_off[multi[j]] = (size_t)used; out_len[multi[j]] = (size_t)((bit + 80 - used * 8 + 7) / 8);
      used += (out_len[multi[j]] + 3) & ~(size_t)3;
    }
    CJS_TRY(DevCache::grow(b.stage, b.stage_cap, used + 16, true, s));
    CJS_HIP_TRY(hipMemsetAsync(b.stage + used0, 0, used - used0 + 16, s));
    DevBuf tb(sizeof(AsmBlock) * ab.size() + sizeof(AsmStream) * as.size() + 64);
    uint8_t* t = (uint8_t*)tb.p;
    if (!t) return CJS_E_OUT_OF_MEMORY;
    AsmBlock* d_ab = (AsmBlock*)t;
    AsmStream* d_as = (AsmStream*)(t + ((sizeof(AsmBlock) * ab.size() + 15) & ~(size_t)15));
    CJS_HIP_TRY(hipMemcpyAsync(d_ab, ab.data(), sizeof(AsmBlock) * ab.size(), hipMemcpyHostToDevice, s));
    CJS_HIP_TRY(hipMemcpyAsync(d_as, as.data(), sizeof(AsmStream) * as.size(), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(batch_asm_blocks, dim3((unsigned)ab.size()), dim3(256), 0, s, d_ab, (const uint32_t*)b.scratch.p, (uint32_t*)b.stage.p);
    hipLaunchKernelGGL(batch_asm_frame, dim3((unsigned)((as.size() + 255) / 256)), dim3(256), 0, s, d_as, (uint32_t)as.size(), level, (uint32_t*)b.stage.p);
    CJS_HIP_TRY(hipGetLastError());
    CJS_HIP_TRY(hipStreamSynchronize(s));
  }
  if (!empty.empty()) {
    CJS_TRY(DevCache::grow(b.stage, b.stage_cap, used + 16 * empty.size(), true, s));
    std::vector<uint64_t> eo(empty.size());
    for (size_t i = 0; i < empty.size(); i++) { eo[i] = used + 16 * i; out_off[empty[i]] = (size_t)eo[i]; out_len[empty[i]] = 14; }
    CJS_HIP_TRY(hipMemcpyAsync(d_len2, eo.data(), 8 * eo.size(), hipMemcpyHostToDevice, s));      // (d_len2 is free again)
    hipLaunchKernelGGL(batch_empty_streams, dim3((unsigned)((eo.size() + 255) / 256)), dim3(256), 0, s, d_len2, (uint32_t)eo.size(), level, (uint32_t*)b.stage.p);
    CJS_HIP_TRY(hipGetLastError());
    CJS_HIP_TRY(hipStreamSynchronize(s));
    used += 16 * empty.size();
  }
  uint64_t last = 0;
  for (size_t k = 0; k < count; k++) last = std::max<uint64_t>(last, (uint64_t)out_off[k] + out_len[k]);
  *end = last;
  if (env_debug()) fprintf(stderr, "[cjs batch] %zu inputs: %u passes (%zu one-block inputs, %zu blocks of %zu inputs of several blocks), %zu empty\n",
                   count, passes, one.size(), parts.size(), multi.size(), empty.size());
  return 0;
}

constexpr size_t BATCH_GROUP_BYTES = (size_t)256 << 20;      // input bytes the host-buffer entry point uploads at a time

}  // namespace cjs

extern "C" int cjs_ctx_create_batch(cjs_ctx** out, int device, size_t max_input, size_t max_items, int level) {
  CJS_GUARD_BEGIN
  if (!out) return CJS_E_INVALID_ARG;
  *out = nullptr;
  if (level < 1 || level > 9) return CJS_E_BAD_LEVEL;
  cjs_ctx* c = nullptr;
  CJS_TRY(cjs_ctx_create_sharded(&c, device, 1, 0, level));        // streams and events; the single-stream workspace stays minimal
  BatchWork* b = new (std::nothrow) BatchWork();
  if (!b) { cjs_ctx_destroy(c); return CJS_E_OUT_OF_MEMORY; }
  c->batch.reset(b);
  if (max_items == 0) max_items = 1;
  b->items = (uint32_t)std::min<size_t>(max_items, BATCH_MAX_ITEMS);
  // slots: the inputs' RLE1 bytes (at most 5/4 of the input) and up to SMALL_SLOT per input for the narrow slots of tiny inputs.
  // The slots left empty behind the shorter blocks of a pass (up to as many again) are not budgeted: a batch that needs them
  // runs in more passes.
  b->elems = std::min<size_t>(std::max<size_t>(max_input + max_input / 4 + (size_t)SMALL_SLOT * b->items, c->cap + 16), BATCH_MAX_ELEMS);
  const size_t segs = Rle1Work::max_segs_for(c->cap) + 2;
  const size_t bytes = BwtWork::bytes_needed(b->elems) + 12 * b->elems + (size_t)b->items * (24576 + 4 * segs + 128) + ((size_t)1 << 20);
  int rc = b->arena.init_pooled(bytes);
  if (!rc && hipHostMalloc((void**)b->h_sc.put(), 64) != hipSuccess) rc = CJS_E_HIP;
  if (rc) { cjs_ctx_destroy(c); return rc; }
  *out = c;
  return 0;
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

extern "C" int cjs_bzip2_compress_batch_device(cjs_ctx* c, const uint8_t* d_in, const size_t* in_off, size_t count, int level, uint8_t* d_out,
                                               size_t out_cap, size_t* out_off, size_t* out_len) {
  clear_detail();
  if (level < 1 || level > 9) return CJS_E_BAD_LEVEL;
  CJS_GUARD_BEGIN
  if (!c || !c->batch || level != c->level || (count && (!in_off || !out_off || !out_len)) || ((uintptr_t)d_out & 3) != 0) return CJS_E_INVALID_ARG;
  if (count == 0) return 0;
  std::vector<uint64_t> st(count), en(count);
  for (size_t k = 0; k < count; k++) {
    if (in_off[k + 1] < in_off[k]) return CJS_E_INVALID_ARG;
    st[k] = in_off[k] - in_off[0]; en[k] = in_off[k + 1] - in_off[0];
  }
  CJS_HIP_TRY(hipSetDevice(c->device));
  uint64_t end = 0;
  int rc = batch_core(c, d_in + in_off[0], st, en, count, level, out_off, out_len, &end);
  if (!rc && end > out_cap) rc = CJS_E_OUTPUT_TOO_SMALL;             // nothing has been written to d_out
  if (!rc && end && hipMemcpyAsync(d_out, c->batch->stage, end, hipMemcpyDeviceToDevice, c->stream) != hipSuccess) rc = CJS_E_HIP;
  if (hipStreamSynchronize(c->stream) != hipSuccess && !rc) rc = CJS_E_HIP;
  return rc;
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

extern "C" int cjs_bzip2_compress_batch(const uint8_t* const* in, const size_t* n, size_t count, int level, uint8_t** out, size_t* off,
                                        size_t* len, const cjs_opts* opts) {
  if (!out) return CJS_E_INVALID_ARG;
  *out = nullptr;
  clear_detail();
  if (level < 1 || level > 9) return CJS_E_BAD_LEVEL;                 // J/Bzip2_joined_.js:2208, before the device is touched
  if (count == 0) return 0;
  if (!in || !n || !off || !len) return CJS_E_INVALID_ARG;
  for (size_t k = 0; k < count; k++) if (n[k] && !in[k]) return CJS_E_INVALID_ARG;
  CJS_GUARD_BEGIN
  CJS_TRY(select_device(opts));
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEVICES) return CJS_E_HIP;
  std::vector<uint8_t> acc;                                             // the streams of all groups, in call order
  std::vector<size_t> goff(count), glen(count);
  int rc = 0;
  {
    CacheLease bc{dev_cache(dev, BATCH_SLOT)};                          // (not slot 0: see host.h)
    std::vector<uint8_t> host_in;
    for (size_t k0 = 0; k0 < count && !rc;) {
      if (n[k0] > BATCH_GROUP_BYTES) {                                   // an input of its own: the single-stream host path
        uint8_t* o = nullptr; size_t on = 0;
        rc = cjs_bzip2_compress(in[k0], n[k0], level, &o, &on, opts);
        if (!rc) { acc.resize((acc.size() + 3) & ~(size_t)3); off[k0] = acc.size(); len[k0] = on; acc.insert(acc.end(), o, o + on); acc.resize((acc.size() + 3) & ~(size_t)3); }
        cjs_free(o);
        k0++;
        continue;
      }
      size_t k1 = k0, bytes = 0;                                        // inputs at 16-byte-aligned offsets (wide loads)
      while (k1 < count && n[k1] <= BATCH_GROUP_BYTES && (k1 == k0 || bytes + n[k1] <= BATCH_GROUP_BYTES)) bytes += (n[k1++] + 15) & ~(size_t)15;
      const size_t items = k1 - k0;
      cjs_ctx*& c = bc.c.ctx;
      if (!c || c->level != level || !c->batch || c->batch->elems < std::min<size_t>(bytes + bytes / 4, BATCH_MAX_ELEMS) ||
          c->batch->items < std::min<size_t>(items, BATCH_MAX_ITEMS)) {
        cjs_ctx_destroy(c); c = nullptr;
        if ((rc = cjs_ctx_create_batch(&c, dev, std::max<size_t>(bytes, 1), items, level)) != 0) break;
      }
      if ((rc = DevCache::grow(bc.c.d_in, bc.c.in_cap, bytes + 16)) != 0) break;
      host_in.resize(bytes + 1);
      std::vector<uint64_t> st(items), en(items);
      for (size_t i = 0, o = 0; i < items; i++) {
        if (n[k0 + i]) memcpy(host_in.data() + o, in[k0 + i], n[k0 + i]);
        st[i] = o; en[i] = o + n[k0 + i]; o += (n[k0 + i] + 15) & ~(size_t)15;
      }
      if (bytes && hipMemcpyAsync(bc.c.d_in, host_in.data(), bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess) { rc = CJS_E_HIP; break; }
      uint64_t total = 0;
      rc = batch_core(c, bc.c.d_in, st, en, items, level, goff.data() + k0, glen.data() + k0, &total);
      if (rc) break;
      const size_t base = (acc.size() + 3) & ~(size_t)3;
      acc.resize(base + total);
      if (total && hipMemcpy(acc.data() + base, c->batch->stage, total, hipMemcpyDeviceToHost) != hipSuccess) { rc = CJS_E_HIP; break; }
      for (size_t i = 0; i < items; i++) { off[k0 + i] = base + goff[k0 + i]; len[k0 + i] = glen[k0 + i]; }
      k0 = k1;
    }
    bc.check(rc);
  }
  if (rc) return rc;
  uint8_t* res = (uint8_t*)HostPool::take(acc.size() ? acc.size() : 1);
  if (!res) return CJS_E_OUT_OF_MEMORY;
  if (!acc.empty()) memcpy(res, acc.data(), acc.size());
  *out = res;
  return 0;
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}
