// radix.hip — segmented LSD radix sorter for gfx950 (8-bit digits, LDS-staged buckets, wave64 match-any ranking).
//
// Sorts n keys of type K (uint64_t / uint32_t), with or without a 32-bit value each, between two buffers, on the whole 8-bit
// digits from lo_bit up that start below hi_bit: bits [lo_bit, lo_bit + 8 * ceil((hi_bit - lo_bit) / 8)), clipped at the key
// width, not [lo_bit, hi_bit) (see radix_passes in cjs_internal.h).  Used by the suffix sort (bwt.hip: round 1, the groups too
// large for the tile sorters, the whole-array fallbacks), by the inverse BWT (dec_ibwt.hip: stable partition of the BWT bytes),
// by the tally (tally.hip) and by the line sort (sort.hip); stage_radix.hip runs it on its own for the tests.  Integer sort/scan
// only (no MFMA); HBM-bound on the scatter passes.
// radix_passes_pk1 is the phase-1 sort of the packed cyclic round 1, five passes on records that shrink as their digits are
// used up: 8 bytes for two passes, then 4 (rs_scatter with a narrower output type, then with its digit from a byte array).
#include "radix.hpp"
#include <type_traits>

namespace cjs {

// ------------------------------------------------------------------------------------------
// LSD radix sort pass: histogram -> per-bin scan over tiles -> stable scatter
// ------------------------------------------------------------------------------------------
// Per-tile digit counts, tile-major: hist[tile * 256 + digit] (one coalesced 1 KB row per workgroup; the digit-major
// layout of round 1 cost a 64-byte memory transaction per 4-byte counter on both sides).
// LDS atomics of one instruction that meet in one address OR in one bank are done one after the other, and text digits
// are skewed (a fifth of the lanes carry a space; a pass over a sorted byte has all 64 lanes on one counter): each wave
// counts into HR = 8 copies of its histogram picked by lane & 7 and laid out digit * 8 + copy, so the copies of a digit
// sit in eight different banks.  100 M keys, MI355X: 237 us (text digit) / 344 us (sorted digit) with one copy per wave;
// copies 1 KB apart (same bank) 141 / 190 us with two and slower again with more; interleaved copies 135 us for both,
// against 125 us for the same loads without any atomic.
constexpr int HR = 8;
template <typename K, bool GEN>
__global__ __launch_bounds__(256) void rs_hist(const K* __restrict__ keys, SegGeom sg, GenSrc gs, int shift,
                                               uint32_t* __restrict__ hist, uint32_t T) {
  __shared__ uint32_t h[4 * 256 * HR];
  __shared__ __attribute__((aligned(16))) uint8_t tb[GEN ? RS_TILE + GEN_PAD + 16 : 16];
  const int tid = threadIdx.x;
  uint32_t* hw = h + (tid >> 6) * 256 * HR + (tid & (HR - 1));          // this lane's copy in this wave's histogram
#pragma unroll
  for (int i = 0; i < 4 * HR; i++) h[i * 256 + tid] = 0;
  const uint32_t tile = blockIdx.x;
  const TileRef t = tile_ref(sg, tile);
  uint32_t tb0 = 0;
  if (GEN) tb0 = gen_stage(gs, sg, t, tb);
  __syncthreads();
  if (GEN) {
#pragma unroll 4
    for (int it = 0; it < 16; it++) {
      const uint32_t loc = (uint32_t)it * 256 + tid;
      if (loc < t.nvalid) atomicAdd(&hw[((uint32_t)(gen_key(gs, sg, t, tb, tb0, loc) >> shift) & 255u) * HR], 1u);
    }
  } else if (t.nvalid) {
    // all sixteen loads are issued before the first atomic (written as one loop the compiler waits for each load in turn)
    K k[16];
#pragma unroll
    for (int it = 0; it < 16; it++) {
      const uint32_t loc = (uint32_t)it * 256 + tid;
      k[it] = keys[t.base + (loc < t.nvalid ? loc : t.nvalid - 1u)];
    }
#pragma unroll
    for (int it = 0; it < 16; it++)
      if ((uint32_t)it * 256 + tid < t.nvalid) atomicAdd(&hw[((uint32_t)((uint64_t)k[it] >> shift) & 255u) * HR], 1u);
  }
  __syncthreads();
  uint32_t sum = 0;
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int r = 0; r < HR; r++) sum += h[i * 256 * HR + tid * HR + r];
  hist[(size_t)tile * 256 + tid] = sum;
}

// The same counts from a byte per key: the scatter pass in front left the NEXT digit of every key it moved in dig[] (same
// index as the key), so this pass reads 1 B per key instead of 8.  Aligned 32-bit loads over the tile's byte range.
// With delta > 0 the bytes are the block TEXT (cyclic form): the first pass's digit of the suffix at position p is the text byte
// at p + delta, so a tile's digits are the text bytes [off + delta, off + delta + nvalid) of its block -- no keys are built for
// the count (rs_hist<GEN>: 130 us); the one tile per block whose range wraps around the block end counts byte by byte.
constexpr int HB = 4;   // histogram copies per wave (the zeroing and folding of 4 * 256 * HB counters is most of this kernel's LDS traffic; 59-82 us per 100 M keys with 4, 72-85 with 8, 75-130 with 2)
__global__ __launch_bounds__(256) void rs_hist_bytes(const uint8_t* __restrict__ dig, SegGeom sg, uint32_t* __restrict__ hist, uint32_t delta) {
  __shared__ uint32_t h[4 * 256 * HB];
  const int tid = threadIdx.x;
  uint32_t* hw = h + (tid >> 6) * 256 * HB + (tid & (HB - 1));
#pragma unroll
  for (int i = 0; i < 4 * HB; i++) h[i * 256 + tid] = 0;
  const uint32_t tile = blockIdx.x;
  const TileRef t = tile_ref(sg, tile);
  const uint32_t sn = t.seg + 1 == sg.nseg ? sg.n_last : sg.stride;
  const bool wraps = delta && t.nvalid && t.off + delta + t.nvalid > sn;         // (wave-uniform)
  if (wraps) {
    __syncthreads();
    const uint8_t* tx = dig + (size_t)t.seg * sg.stride;
    for (uint32_t e = tid; e < t.nvalid; e += 256) atomicAdd(&hw[(uint32_t)tx[(t.off + e + delta) % sn] * HB], 1u);
  }
  const uintptr_t a0 = (uintptr_t)(dig + t.base + delta), a1 = a0 + (wraps ? 0u : t.nvalid);
  const uint32_t* al = reinterpret_cast<const uint32_t*>(a0 & ~(uintptr_t)3);
  uint32_t wv[5];
#pragma unroll
  for (int j = 0; j < 5; j++) {
    const uint32_t wi = (uint32_t)j * 256u + tid;
    wv[j] = (t.nvalid && (uintptr_t)(al + wi) < a1) ? al[wi] : 0u;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 5; j++) {
    const uintptr_t wa = (uintptr_t)(al + ((uint32_t)j * 256u + tid));
#pragma unroll
    for (int b = 0; b < 4; b++)
      if (wa + b >= a0 && wa + b < a1) atomicAdd(&hw[((wv[j] >> (8 * b)) & 255u) * HB], 1u);
  }
  __syncthreads();
  uint32_t sum = 0;
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int r = 0; r < HB; r++) sum += h[i * 256 * HB + tid * HB + r];
  hist[(size_t)tile * 256 + tid] = sum;
}

// one workgroup per segment: exclusive scan over the segment's tiles of every digit's count (thread = digit; the rows are
// read coalesced and the loads of a batch are independent, only the running sums are a chain); digit totals -> bintot
__global__ __launch_bounds__(256) void rs_scan_bins(uint32_t* __restrict__ hist, uint32_t tps, uint32_t* __restrict__ bintot) {
  uint32_t* p = hist + (size_t)blockIdx.x * tps * 256 + threadIdx.x;
  uint32_t carry = 0;
  uint32_t i = 0;
  for (; i + 8 <= tps; i += 8) {
    uint32_t v[8];
#pragma unroll
    for (int j = 0; j < 8; j++) v[j] = p[(size_t)(i + j) * 256];
#pragma unroll
    for (int j = 0; j < 8; j++) { p[(size_t)(i + j) * 256] = carry; carry += v[j]; }
  }
  for (; i < tps; i++) { const uint32_t v = p[(size_t)i * 256]; p[(size_t)i * 256] = carry; carry += v; }
  bintot[(size_t)blockIdx.x * 256 + threadIdx.x] = carry;
}
// plain (one-segment) sorts have up to tens of thousands of tiles: three-phase scan, chunks of SB_CHUNK tiles
constexpr uint32_t SB_CHUNK = 64;
__global__ __launch_bounds__(256) void rs_scan_chunk_sum(const uint32_t* __restrict__ hist, uint32_t T, uint32_t* __restrict__ csum) {
  const uint32_t t0 = blockIdx.x * SB_CHUNK, t1 = t0 + SB_CHUNK < T ? t0 + SB_CHUNK : T;
  uint32_t acc = 0;
  for (uint32_t t = t0; t < t1; t++) acc += hist[(size_t)t * 256 + threadIdx.x];
  csum[(size_t)blockIdx.x * 256 + threadIdx.x] = acc;
}
__global__ __launch_bounds__(256) void rs_scan_chunk_mid(uint32_t* __restrict__ csum, uint32_t nch, uint32_t* __restrict__ bintot) {
  uint32_t carry = 0;
  for (uint32_t c = 0; c < nch; c++) { const uint32_t v = csum[(size_t)c * 256 + threadIdx.x]; csum[(size_t)c * 256 + threadIdx.x] = carry; carry += v; }
  bintot[threadIdx.x] = carry;
}
__global__ __launch_bounds__(256) void rs_scan_chunk_apply(uint32_t* __restrict__ hist, uint32_t T, const uint32_t* __restrict__ csum) {
  const uint32_t t0 = blockIdx.x * SB_CHUNK, t1 = t0 + SB_CHUNK < T ? t0 + SB_CHUNK : T;
  uint32_t carry = csum[(size_t)blockIdx.x * 256 + threadIdx.x];
  for (uint32_t t = t0; t < t1; t++) { const uint32_t v = hist[(size_t)t * 256 + threadIdx.x]; hist[(size_t)t * 256 + threadIdx.x] = carry; carry += v; }
}

// KO: the records as they go out -- K, or the narrow phase-1 record (pk1_of, bwt_rules.h) of a packed one; they are staged in
// LDS as they come in.  DIGIN (key-only passes): the records no longer hold this pass's digit: it is the byte that the pass in
// front left at the record's index, handed in through vin and staged beside the records (a byte each); such a pass leaves no
// digit for the next one -- other workgroups of the launch are still reading the array it would write to.  Otherwise the digit
// is bits [shift, shift + 8) and the next one lies above it.
template <typename K, bool GEN, bool NOVAL, typename KO = K, bool DIGIN = false>
__global__ __launch_bounds__(256) void rs_scatter(const K* __restrict__ kin, const std::conditional_t<DIGIN, uint8_t, uint32_t>* __restrict__ vin,
                                                  KO* __restrict__ kout, uint32_t* __restrict__ vout, SegGeom sg, GenSrc gs, int shift,
                                                  const uint32_t* __restrict__ hist, uint32_t T, const uint32_t* __restrict__ bintot,
                                                  uint8_t* __restrict__ dig /* next digit of every key, at the key's new index (or null) */) {
  __shared__ __attribute__((aligned(16))) K skey[RS_TILE + 2];
  __shared__ uint32_t sval[NOVAL ? 1 : RS_TILE];
  __shared__ uint8_t sdig[DIGIN ? RS_TILE : 1];
  __shared__ uint32_t wcnt[4][256];
  __shared__ uint32_t goff[256];
  __shared__ uint32_t sm[4];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const uint32_t tile = blockIdx.x;
  const TileRef t = tile_ref(sg, tile);
  const uint64_t base = t.base;
  const uint32_t nvalid = t.nvalid;
  for (int i = tid; i < 1024; i += 256) (&wcnt[0][0])[i] = 0;
  static_assert(!DIGIN || (NOVAL && !GEN), "the digit bytes come in where the values would");
  K k[16];
  uint32_t v[16];
  uint32_t rk[16];
  if (GEN) {
    uint8_t* tb = reinterpret_cast<uint8_t*>(skey);     // skey is not written before the ranking is done
    const uint32_t tb0 = gen_stage(gs, sg, t, tb);
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 16; s++) {
      const uint32_t loc = (uint32_t)w * 1024u + (uint32_t)s * 64u + lane;
      const bool ok = loc < nvalid;
      k[s] = ok ? (K)gen_key(gs, sg, t, tb, tb0, loc) : (K)~(K)0;
      v[s] = ok ? t.off + loc : 0u;
    }
  } else {
#pragma unroll
    for (int s = 0; s < 16; s++) {
      const uint32_t loc = (uint32_t)w * 1024u + (uint32_t)s * 64u + lane;
      const bool ok = loc < nvalid;
      k[s] = ok ? kin[base + loc] : (K)~(K)0;           // (non-temporal loads here: no change, 12.69 vs 12.69 ms per step)
      if constexpr (DIGIN) v[s] = ok ? (uint32_t)vin[base + loc] : 255u;      // v[] = this pass's digit
      else v[s] = (ok && !NOVAL) ? vin[base + loc] : 0u;
    }
  }
  __syncthreads();
#pragma unroll
  for (int s = 0; s < 16; s++) {
    if constexpr (DIGIN) rk[s] = rank_step(v[s], wcnt[w]);
    else rk[s] = rank_step((uint32_t)(k[s] >> shift) & 255u, wcnt[w]);
  }
  __syncthreads();
  {
    const uint32_t c0 = wcnt[0][tid], c1 = wcnt[1][tid], c2 = wcnt[2][tid], c3 = wcnt[3][tid];
    uint32_t total;
    const uint32_t ex = block_excl_sum<256>(c0 + c1 + c2 + c3, sm, total);
    uint32_t tot2;
    const uint32_t binbase = block_excl_sum<256>(bintot[(size_t)t.seg * 256 + tid], sm, tot2);
    wcnt[0][tid] = ex; wcnt[1][tid] = ex + c0; wcnt[2][tid] = ex + c0 + c1; wcnt[3][tid] = ex + c0 + c1 + c2;
    goff[tid] = t.seg * sg.stride + binbase + hist[(size_t)tile * 256 + tid] - ex;
  }
  __syncthreads();
#pragma unroll
  for (int s = 0; s < 16; s++) {
    uint32_t d;
    if constexpr (DIGIN) d = v[s]; else d = (uint32_t)(k[s] >> shift) & 255u;
    const uint32_t p = wcnt[w][d] + rk[s];
    skey[p] = k[s];
    if (!NOVAL) sval[p] = v[s];
    if constexpr (DIGIN) sdig[p] = (uint8_t)d;
  }
  __syncthreads();
#pragma unroll 4
  for (int it = 0; it < 16; it++) {
    const uint32_t j = (uint32_t)it * 256u + tid;
    if (j < nvalid) {
      const K kk = skey[j];
      uint32_t dst;
      if constexpr (DIGIN) dst = goff[sdig[j]] + j; else dst = goff[(uint32_t)(kk >> shift) & 255u] + j;
      if constexpr (sizeof(KO) < sizeof(K)) kout[dst] = pk1_of(kk); else kout[dst] = kk;
      if (!NOVAL) vout[dst] = sval[j];
      if constexpr (!DIGIN) if (dig) dig[dst] = (uint8_t)((uint64_t)kk >> (shift + 8));
    }
  }
}

// the tile counts of a digit in w.hist -> every tile's offsets inside its segment, digit totals per segment in w.bintot
static void scan_counts(hipStream_t s, RadixWork& w, const SegGeom& sg) {
  if (sg.tps <= 4 * SB_CHUNK) { hipLaunchKernelGGL(rs_scan_bins, dim3(sg.nseg), dim3(256), 0, s, w.hist, sg.tps, w.bintot); return; }
  for (uint32_t sgi = 0; sgi < sg.nseg; sgi++) {      // one long segment (nseg > 1 with long segments: still correct, one launch per segment)
    uint32_t* hseg = w.hist + (size_t)sgi * sg.tps * 256;
    const uint32_t nch = (sg.tps + SB_CHUNK - 1) / SB_CHUNK;
    uint32_t* csum = w.hist + (size_t)w.hist_tiles * 256;          // behind the per-tile rows (RadixWork::hist_words)
    hipLaunchKernelGGL(rs_scan_chunk_sum, dim3(nch), dim3(256), 0, s, hseg, sg.tps, csum);
    hipLaunchKernelGGL(rs_scan_chunk_mid, dim3(1), dim3(256), 0, s, csum, nch, w.bintot + (size_t)sgi * 256);
    hipLaunchKernelGGL(rs_scan_chunk_apply, dim3(nch), dim3(256), 0, s, hseg, sg.tps, csum);
  }
}

// (declared in cjs_internal.h) first_hist_ready: w.hist already holds the tile counts of the first digit; dig: byte per key for
// the next pass's counts (see rs_hist_bytes)
template <typename K>
int radix_passes(hipStream_t s, RadixWork& w, K* k0, uint32_t* v0, K* k1, uint32_t* v1, int& cur, uint32_t n, int lo_bit, int hi_bit,
                 LaunchTimes* lt, const SegGeom* seg, const GenSrc* gen, bool noval, bool first_hist_ready, uint8_t* dig) {
  const uint32_t T1 = (n + RS_TILE - 1) / RS_TILE;
  const SegGeom sg = seg ? *seg : SegGeom{1u, n, n, T1};
  const uint32_t T = sg.nseg * sg.tps;
  if (T > w.hist_tiles || sg.nseg > w.bintot_segs) return CJS_E_INVALID_ARG;
  K* kk[2] = {k0, k1}; uint32_t* vv[2] = {v0, v1};
  const GenSrc g0{nullptr, 0, 0, 0};
  for (int shift = lo_bit; shift < hi_bit; shift += 8) {
    const bool first_gen = gen && shift == lo_bit;        // the first pass makes its keys from the block bytes
    const bool dig_out = dig && shift + 8 < hi_bit;          // a pass follows: leave its digits
    if (first_hist_ready && shift == lo_bit) {}
    else if (dig && shift != lo_bit) hipLaunchKernelGGL(rs_hist_bytes, dim3(T), dim3(256), 0, s, dig, sg, w.hist, 0u);
    else if (first_gen && gen->cyclic && gen->packed && shift == PK_KEY_LO)       // packed cyclic sort: the first digit is the text byte at suffix + 6
      hipLaunchKernelGGL(rs_hist_bytes, dim3(T), dim3(256), 0, s, gen->T, sg, w.hist, 6u);
    else if (first_gen) hipLaunchKernelGGL((rs_hist<K, true>), dim3(T), dim3(256), 0, s, kk[cur], sg, *gen, shift, w.hist, T);
    else hipLaunchKernelGGL((rs_hist<K, false>), dim3(T), dim3(256), 0, s, kk[cur], sg, g0, shift, w.hist, T);
    scan_counts(s, w, sg);
    if (lt) lt->begin(s, n);
#define RS_SCATTER(GEN_, NOVAL_, G_) hipLaunchKernelGGL((rs_scatter<K, GEN_, NOVAL_>), dim3(T), dim3(256), 0, s, kk[cur], vv[cur], kk[1 - cur], vv[1 - cur], sg, G_, shift, w.hist, T, w.bintot, dig_out ? dig : nullptr)
    if (noval) { if (first_gen) RS_SCATTER(true, true, *gen); else RS_SCATTER(false, true, g0); }
    else { if (first_gen) RS_SCATTER(true, false, *gen); else RS_SCATTER(false, false, g0); }
#undef RS_SCATTER
    if (lt) lt->end(s);
    cur = 1 - cur;
  }
  CJS_HIP_TRY(hipGetLastError());
  return 0;
}
template int radix_passes<uint64_t>(hipStream_t, RadixWork&, uint64_t*, uint32_t*, uint64_t*, uint32_t*, int&, uint32_t, int, int, LaunchTimes*,
                                    const SegGeom*, const GenSrc*, bool, bool, uint8_t*);
template int radix_passes<uint32_t>(hipStream_t, RadixWork&, uint32_t*, uint32_t*, uint32_t*, uint32_t*, int&, uint32_t, int, int, LaunchTimes*,
                                    const SegGeom*, const GenSrc*, bool, bool, uint8_t*);

int radix_pass_segments(hipStream_t s, RadixWork& w, uint32_t* k0, uint32_t* v0, uint32_t* k1, uint32_t* v1, int& cur, uint32_t nseg, uint32_t stride,
                        int lo_bit, int hi_bit, bool noval, bool first_hist_ready) {
  const SegGeom sg{nseg, stride, stride, (stride + RS_TILE - 1) / RS_TILE};
  return radix_passes<uint32_t>(s, w, k0, v0, k1, v1, cur, nseg * stride, lo_bit, hi_bit, nullptr, &sg, nullptr, noval, first_hist_ready);
}

// (declared in cjs_internal.h)  Pass by pass, what a record still has to carry shrinks: passes 1 and 2 (bytes 6, 5) move the
// 8-byte pk_record; pass 3 (byte 4) reads it and writes the 4-byte pk1 record, byte 3 beside it in dig[] as every pass leaves the
// next digit; pass 4 takes its digit from dig[] at the record's own index and leaves none (see rs_scatter); pass 5 (byte 2, in
// the record) is the plain 32-bit key-only pass and counts its digits from the records.
int radix_passes_pk1(hipStream_t s, RadixWork& w, uint64_t* k0, uint64_t* k1, uint32_t* n0, uint32_t* n1, uint32_t n, LaunchTimes* lt,
                     const SegGeom& sg, const GenSrc& gen, uint8_t* dig) {
  const uint32_t T = sg.nseg * sg.tps;
  if (T > w.hist_tiles || sg.nseg > w.bintot_segs) return CJS_E_INVALID_ARG;
  const GenSrc g0{nullptr, 0, 0, 0};
  // counts of the pass's digit from a byte per record (pass 1: the text byte at suffix + 6), then their scan; the scatter is timed
  auto counts = [&](const uint8_t* bytes, uint32_t delta) {
    hipLaunchKernelGGL(rs_hist_bytes, dim3(T), dim3(256), 0, s, bytes, sg, w.hist, delta);
    scan_counts(s, w, sg);
    if (lt) lt->begin(s, n);
  };
  counts(gen.T, 6u);
  hipLaunchKernelGGL((rs_scatter<uint64_t, true, true>), dim3(T), dim3(256), 0, s, k0, nullptr, k0, nullptr, sg, gen, PK_KEY_LO, w.hist, T, w.bintot, dig);
  if (lt) lt->end(s);
  counts(dig, 0u);
  hipLaunchKernelGGL((rs_scatter<uint64_t, false, true>), dim3(T), dim3(256), 0, s, k0, nullptr, k1, nullptr, sg, g0, PK_KEY_LO + 8, w.hist, T, w.bintot, dig);
  if (lt) lt->end(s);
  counts(dig, 0u);
  hipLaunchKernelGGL((rs_scatter<uint64_t, false, true, uint32_t>), dim3(T), dim3(256), 0, s, k1, nullptr, n0, nullptr, sg, g0, PK_KEY_LO + 16, w.hist, T, w.bintot, dig);
  if (lt) lt->end(s);
  counts(dig, 0u);
  hipLaunchKernelGGL((rs_scatter<uint32_t, false, true, uint32_t, true>), dim3(T), dim3(256), 0, s, n0, dig, n1, nullptr, sg, g0, 0, w.hist, T, w.bintot, nullptr);
  if (lt) lt->end(s);
  hipLaunchKernelGGL((rs_hist<uint32_t, false>), dim3(T), dim3(256), 0, s, n1, sg, g0, PK1_B2_SHIFT, w.hist, T);
  scan_counts(s, w, sg);
  if (lt) lt->begin(s, n);
  hipLaunchKernelGGL((rs_scatter<uint32_t, false, true>), dim3(T), dim3(256), 0, s, n1, nullptr, n0, nullptr, sg, g0, PK1_B2_SHIFT, w.hist, T, w.bintot, nullptr);
  if (lt) lt->end(s);
  CJS_HIP_TRY(hipGetLastError());
  return 0;
}

int RadixWork::carve(Arena& a, size_t tiles, size_t segs) {
  hist_tiles = (uint32_t)tiles; bintot_segs = (uint32_t)segs;
  hist = a.take<uint32_t>(hist_words(tiles)); bintot = a.take<uint32_t>(256 * segs);
  return hist && bintot ? 0 : CJS_E_OUT_OF_MEMORY;
}

}  // namespace cjs
