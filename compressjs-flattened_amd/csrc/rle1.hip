// rle1.hip — bzip2 stage 0a on the GPU: the block boundaries of a stream under RLE1 (tile tables, their scans, the boundary
// walk) and the stage's workspace.  The RLE1 bytes: rle1_bytes.hip; batches of inputs: rle1_batch.hip; the block CRCs: crc.hip;
// the rules of the arithmetic: rle1_rules.h; the device helpers: rle1_dev.hpp.
//
// Replaces readBlock (J/Bzip2_joined_.js:1954-1985) + CRC32.updateCRC (:1048-1079) + the block
// loop's use of them (:2233-2242).  The reference walks the input byte-serially; block k+1 starts
// where block k's RLE1 OUTPUT reached level*100000-19 bytes and the run-chunking state is reset at
// every block start.  Parallel formulation used here:
//   c[i]  = bytes emitted when input byte i is consumed, under the "global" chunking (chunks of
//           <= 255 equal bytes counted from the start of each maximal run):
//           offset-in-chunk d' = (i - runstart) % 255 : d'<3 -> 1 (literal), d'==3 -> 2 (literal +
//           count byte), d'>=4 -> 0 (absorbed into the count byte)
//   G     = exclusive prefix sum of c (per 4096-byte tile: G_tile, then in-tile scan)
//   a block that starts at s re-chunks only the run that contains s (closed form); after that
//   run the global chunking applies again, so its end is found by a search on G.
// Kernels: tile summaries -> tile scans -> serial-over-blocks walk by ONE workgroup (k-ary search
// over G_tile + in-tile scan; O(#blocks) steps) -> materialise RLE1 bytes -> CRC (slice + GF(2)
// combine).  Integer/byte work, HBM-bound streaming reads.
#include "rle1_dev.hpp"
#include "rle1.h"

namespace cjs {

// ---- P1: per tile first / last boundary (global position + 1; 0 = none)
__global__ __launch_bounds__(256) void rle_tile_summary(const uint8_t* __restrict__ in, uint64_t N, uint64_t* __restrict__ fb, uint64_t* __restrict__ lb, uint32_t t0) {
  __shared__ uint32_t smin[4], smax[4];
  const uint32_t tile = t0 + blockIdx.x;
  const uint64_t tile_start = (uint64_t)tile * RT, p0 = tile_start + (uint64_t)threadIdx.x * 16;
  uint8_t b[16];
  uint32_t last;
  const uint32_t bm = boundaries16(in, N, p0, N, b, last), rel0 = (uint32_t)threadIdx.x * 16u;
  uint32_t first = bm ? rel0 + (uint32_t)__builtin_ctz(bm) : 0xFFFFFFFFu;
  if (last) last += rel0;
  first = wave_min(first); last = wave_max(last);
  if (lane_id() == 0) { smin[wave_id()] = first; smax[wave_id()] = last; }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t f = smin[0], l = smax[0];
    for (int i = 1; i < 4; i++) { f = smin[i] < f ? smin[i] : f; l = smax[i] > l ? smax[i] : l; }
    fb[tile] = f == 0xFFFFFFFFu ? 0 : tile_start + f + 1;
    lb[tile] = l ? tile_start + l : 0;     // (tile_start + l-1) + 1
  }
}

// ---- P2: run_start_in[t] = start of the run containing the tile's first byte (from earlier tiles);
//          next_bnd[t] = first boundary in later tiles (N if none): rle_scanb_* below (three-phase scans)

// ---- P3: per-tile emitted byte count under the global chunking, plus two small tables per 256-byte subtile
//          (used by the speculative boundary search): subpre = emitted bytes of the tile before the subtile,
//          dmod = chunk phase (offset in run mod 255) of the subtile's first byte
__global__ __launch_bounds__(256) void rle_tile_count(const uint8_t* __restrict__ in, uint64_t N, const uint64_t* __restrict__ run_start_in,
                                                      uint64_t* __restrict__ gt, uint16_t* __restrict__ subpre, uint8_t* __restrict__ dmod, uint32_t t0) {
  __shared__ uint32_t smem[256 + 16];
  const uint32_t tile = t0 + blockIdx.x;
  const uint64_t tile_start = (uint64_t)tile * RT;
  uint8_t b[16]; uint32_t bm; uint64_t rs;
  run_starts<256, 16>(in, N, tile_start, run_start_in[tile], smem, b, bm, rs);
  const uint64_t p0 = tile_start + (uint64_t)threadIdx.x * 16;
  if ((threadIdx.x & 15) == 0) dmod[(size_t)tile * 16 + (threadIdx.x >> 4)] = (uint8_t)(p0 < N ? (((bm & 1u) ? 0ull : p0 - rs) % 255) : 0);
  uint32_t dpv[16];
  const uint32_t cnt = emit16(p0, N, rs, bm, dpv);
  uint32_t tot;
  const uint32_t ex = block_excl_sum<256>(cnt, smem, tot);
  if ((threadIdx.x & 15) == 0) subpre[(size_t)tile * 16 + (threadIdx.x >> 4)] = (uint16_t)ex;
  if (threadIdx.x == 0) gt[tile] = tot;
}

// ---- P4: exclusive prefix sum (u64) over tiles, one workgroup; gt[Tn] = total
// ---- the tile scans (P2, and the exclusive prefix of the per-tile emitted counts) as three-phase scans over chunks of
//      1024 tiles (reduce -> scan of the chunk aggregates -> apply), so that their time does not grow with the stream (a multi-GPU job replicates this pass on every rank).
//      agg: [0..nch) chunk max of lb, [nch..2nch) chunk max of the inverted fb, [2nch..3nch) chunk sum of gt
constexpr uint32_t SC = 1024;
__global__ __launch_bounds__(1024) void rle_scanb_reduce(const uint64_t* __restrict__ fb, const uint64_t* __restrict__ lb, uint32_t Tn,
                                                         unsigned long long* __restrict__ agg, uint32_t nch) {
  __shared__ unsigned long long sm[16];
  const uint32_t i = blockIdx.x * SC + threadIdx.x;
  const unsigned long long l = i < Tn ? lb[i] : 0ull, f = i < Tn ? fb[i] : 0ull;
  const unsigned long long ml = block_incl_max<1024>(l, sm);
  const unsigned long long mf = block_incl_max<1024>(f ? (NONE64 - f) : 0ull, sm);
  if (threadIdx.x == 1023) { agg[blockIdx.x] = ml; agg[nch + blockIdx.x] = mf; }
}
// single workgroup: exclusive prefix max of agg[0..nch), exclusive SUFFIX max of agg[nch..2nch)
__global__ __launch_bounds__(1024) void rle_scanb_mid(unsigned long long* __restrict__ agg, uint32_t nch) {
  __shared__ unsigned long long sm[16];
  __shared__ unsigned long long arr[1024];
  unsigned long long carry = 0;
  for (uint32_t base = 0; base < nch; base += 1024) {
    const uint32_t i = base + threadIdx.x;
    const unsigned long long v = i < nch ? agg[i] : 0ull;
    const unsigned long long im = block_incl_max<1024>(v, sm);
    arr[threadIdx.x] = im;
    __syncthreads();
    const unsigned long long prev = threadIdx.x ? arr[threadIdx.x - 1] : 0ull, cmx = arr[1023];
    __syncthreads();
    if (i < nch) agg[i] = prev > carry ? prev : carry;
    carry = cmx > carry ? cmx : carry;
  }
  unsigned long long scarry = 0;
  const uint32_t rounds = (nch + 1023) / 1024;
  for (uint32_t r = 0; r < rounds; r++) {
    const uint32_t base = (rounds - 1 - r) * 1024;
    const uint32_t i = base + (1023 - threadIdx.x);
    const unsigned long long v = i < nch ? agg[nch + i] : 0ull;
    const unsigned long long im = block_incl_max<1024>(v, sm);
    arr[threadIdx.x] = im;
    __syncthreads();
    const unsigned long long prev = threadIdx.x ? arr[threadIdx.x - 1] : 0ull, cmx = arr[1023];
    __syncthreads();
    if (i < nch) agg[nch + i] = prev > scarry ? prev : scarry;
    scarry = cmx > scarry ? cmx : scarry;
  }
}
// carry[0] = (last boundary in front of the scanned tile range) + 1, 0 = none; carry[1] = first boundary behind the range, N = none
// (a rank of a multi-GPU job scans only its share of the tiles: rle_probe finds the two)
__global__ __launch_bounds__(1024) void rle_scanb_apply(uint64_t* __restrict__ fb, uint64_t* __restrict__ lb, uint32_t Tn,
                                                        const unsigned long long* __restrict__ agg, uint32_t nch, const uint64_t* __restrict__ carry_io) {
  __shared__ unsigned long long sm[16];
  __shared__ unsigned long long arr[1024];
  {                                                              // run start of each tile's first byte: exclusive prefix max of lb
    const uint32_t i = blockIdx.x * SC + threadIdx.x;
    const unsigned long long carry = agg[blockIdx.x];
    const unsigned long long v = i < Tn ? lb[i] : 0ull;
    const unsigned long long im = block_incl_max<1024>(v, sm);
    arr[threadIdx.x] = im;
    __syncthreads();
    const unsigned long long prev = threadIdx.x ? arr[threadIdx.x - 1] : 0ull;
    __syncthreads();
    if (i < Tn) { unsigned long long e = prev > carry ? prev : carry; const unsigned long long c0 = carry_io[0]; e = e > c0 ? e : c0; lb[i] = e ? e - 1 : 0ull; }
  }
  {                                                              // next boundary after each tile: exclusive suffix min of fb
    const uint32_t i = blockIdx.x * SC + (1023 - threadIdx.x);
    const unsigned long long scarry = agg[nch + blockIdx.x];
    const unsigned long long f = i < Tn ? fb[i] : 0ull;
    const unsigned long long im = block_incl_max<1024>(f ? (NONE64 - f) : 0ull, sm);
    arr[threadIdx.x] = im;
    __syncthreads();
    const unsigned long long prev = threadIdx.x ? arr[threadIdx.x - 1] : 0ull;
    __syncthreads();
    if (i < Tn) { const unsigned long long e = prev > scarry ? prev : scarry; fb[i] = e ? (NONE64 - e) - 1 : carry_io[1]; }
  }
}
__global__ __launch_bounds__(1024) void rle_scanc_reduce(const uint64_t* __restrict__ gt, uint32_t Tn, unsigned long long* __restrict__ agg, uint32_t nch) {
  __shared__ unsigned long long sm[16];
  const uint32_t i = blockIdx.x * SC + threadIdx.x;
  const unsigned long long t = block_sum<1024>((unsigned long long)(i < Tn ? gt[i] : 0ull), sm);
  if (threadIdx.x == 0) agg[2 * nch + blockIdx.x] = t;
}
__global__ __launch_bounds__(1024) void rle_scanc_mid(unsigned long long* __restrict__ agg, uint32_t nch, uint64_t* __restrict__ gt, uint32_t Tn) {
  __shared__ unsigned long long sm[16];
  unsigned long long carry = 0;
  for (uint32_t base = 0; base < nch; base += 1024) {
    const uint32_t i = base + threadIdx.x;
    unsigned long long v = i < nch ? agg[2 * nch + i] : 0ull, tot;
    const unsigned long long ex = block_excl_sum<1024>(v, sm, tot);
    if (i < nch) agg[2 * nch + i] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) gt[Tn] = carry;
}
__global__ __launch_bounds__(1024) void rle_scanc_apply(uint64_t* __restrict__ gt, uint32_t Tn, const unsigned long long* __restrict__ agg, uint32_t nch) {
  __shared__ unsigned long long sm[16];
  const uint32_t i = blockIdx.x * SC + threadIdx.x;
  unsigned long long v = i < Tn ? gt[i] : 0ull, tot;
  const unsigned long long ex = block_excl_sum<1024>(v, sm, tot);
  if (i < Tn) gt[i] = agg[2 * nch + blockIdx.x] + ex;
}

// in-tile helper for the walk (1024 threads x 4 positions): inclusive prefix of c at each position.
// Returns via `firstpos` the smallest position p in the tile with gbase + incl(p) >= target (NONE64 if none),
// and via `upto_sum` the sum of c over positions < upto.
__device__ void walk_tile_eval(const uint8_t* __restrict__ in, uint64_t N, uint64_t tile_start, uint64_t carry, uint64_t gbase,
                               uint64_t target, uint64_t upto, uint32_t* smem, unsigned long long* sh64,
                               uint64_t& firstpos, uint32_t& upto_sum) {
  uint8_t b[4]; uint32_t bm; uint64_t rs;
  run_starts<1024, 4>(in, N, tile_start, carry, smem, b, bm, rs);
  const uint64_t p0 = tile_start + (uint64_t)threadIdx.x * 4;
  uint32_t c[4], cnt = 0, below = 0;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const uint64_t p = p0 + j;
    c[j] = 0;
    if (p < N) {
      if ((bm >> j) & 1u) rs = p;
      c[j] = chunk_emit((uint32_t)((p - rs) % 255));
      cnt += c[j];
      if (p < upto) below += c[j];
    }
  }
  uint32_t tot;
  uint32_t ex = block_excl_sum<1024>(cnt, smem, tot);
  upto_sum = block_sum<1024>(below, smem);
  if (threadIdx.x == 0) sh64[0] = NONE64;
  __syncthreads();
  unsigned long long mine = NONE64;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const uint64_t p = p0 + j;
    ex += c[j];
    if (p < N && mine == NONE64 && c[j] && gbase + ex >= target) mine = p;
  }
  if (mine != NONE64) atomicMin(&sh64[0], mine);
  __syncthreads();
  firstpos = sh64[0];
  __syncthreads();
}

// ---- W: block boundaries.  ONE workgroup, serial over blocks.
// Speculative boundary search: from a block start s0 that coincides with a run boundary (fresh chunking == global
// chunking), the next boundaries are where G reaches G(s0) + j*cap.  Group j (32 lanes) looks boundary j up
// (search on G_tile, then the subtile table, then the <= 256 bytes of the subtile).  A boundary is "clean" when G hits
// the target exactly and the next block again starts on a run boundary; blocks up to the first unclean boundary
// are exact; the next round then starts inside a run (see rle_walk).
struct SpecOut { uint64_t e; uint32_t clean; uint32_t eof; uint32_t len_last; };
// The search for ONE target is done by a group of 32 lanes: 32-ary search on G_tile (3 dependent loads instead of the
// 15 of a binary search), one ballot over the 16 subtile prefixes, and the 256-byte subtile scanned 8 bytes per lane with two
// 32-lane scans (last run start, emitted-byte prefix).  A round of the walk costs a handful of memory round trips.
__device__ SpecOut spec_boundary_group(const uint8_t* __restrict__ in, uint64_t N, uint32_t Tn, const uint64_t* __restrict__ gt,
                                       const uint16_t* __restrict__ subpre, const uint8_t* __restrict__ dmod, uint64_t target, uint64_t prev_target) {
  const uint32_t l = threadIdx.x & 31u, hs = threadIdx.x & 32u;        // lane in the group; the group's half of the wave ballot
  SpecOut o; o.e = N; o.clean = 0; o.eof = 0; o.len_last = 0;
  const uint64_t gtot = gt[Tn];
  if (gtot < target) { o.eof = 1; o.len_last = gtot > prev_target ? (uint32_t)(gtot - prev_target) : 0u; return o; }
  uint32_t lo = 0, hi = Tn;                       // gt[lo] < target <= gt[hi]
  while (hi - lo > 1) {
    const uint32_t step = (hi - lo + 31u) / 32u;
    const uint64_t idx = (uint64_t)lo + (uint64_t)l * step;
    const bool pred = idx < hi && gt[idx] < target;
    const uint32_t cnt = (uint32_t)__builtin_popcount((uint32_t)(__ballot(pred) >> hs));     // ones are a prefix (gt is monotone), lane 0 is one
    const uint32_t nlo = lo + (cnt - 1u) * step;
    hi = nlo + step < hi ? nlo + step : hi;
    lo = nlo;
  }
  const uint64_t need = target - gt[lo];          // 1 .. tile count
  const uint32_t sp = l < 16 ? (uint32_t)subpre[(size_t)lo * 16 + l] : 0u;
  const bool pq = l < 16 && (l == 0 || (uint64_t)sp < need);
  const uint32_t sb = (uint32_t)__builtin_popcount((uint32_t)(__ballot(pq) >> hs)) - 1u;
  const uint32_t acc0 = (uint32_t)__shfl((int)sp, (int)sb, 32);
  const uint32_t d0 = dmod[(size_t)lo * 16 + sb];
  const uint64_t p0 = (uint64_t)lo * RT + (uint64_t)sb * 256;
  const uint64_t pb = p0 + 8u * l;
  uint8_t b[8];
  if (pb + 8 <= N && (((uintptr_t)(in + pb)) & 7u) == 0) {
    const uint64_t v = *reinterpret_cast<const uint64_t*>(in + pb);
#pragma unroll
    for (int t = 0; t < 8; t++) b[t] = (uint8_t)(v >> (8 * t));
  } else {
#pragma unroll
    for (int t = 0; t < 8; t++) b[t] = pb + t < N ? in[pb + t] : 0;
  }
  const uint32_t prevb = (uint32_t)__shfl_up((int)b[7], 1, 32);
  uint32_t rsmask = 0; int my_last = -1;
#pragma unroll
  for (int t = 0; t < 8; t++) {
    const uint32_t i = 8u * l + t;
    const uint32_t pv = t ? b[t - 1] : prevb;
    if (i > 0 && pb + t < N && b[t] != pv) { rsmask |= 1u << t; my_last = (int)i; }
  }
  int incl = my_last;
#pragma unroll
  for (int d = 1; d < 32; d <<= 1) { const int x = __shfl_up(incl, d, 32); if ((int)l >= d && x > incl) incl = x; }
  int rs = __shfl_up(incl, 1, 32);
  if (l == 0) rs = -1;
  uint32_t cs[8], sum = 0;
#pragma unroll
  for (int t = 0; t < 8; t++) {
    const uint32_t i = 8u * l + t;
    if ((rsmask >> t) & 1u) rs = (int)i;
    uint32_t dm = rs >= 0 ? i - (uint32_t)rs : d0 + i;
    dm = dm >= 255u ? dm - 255u : dm;                                   // d0 <= 254, i <= 255: one subtract is "% 255"
    dm = dm >= 255u ? dm - 255u : dm;
    const uint32_t c = pb + t < N ? chunk_emit(dm) : 0u;
    sum += c; cs[t] = sum;
  }
  uint32_t incl2 = sum;
#pragma unroll
  for (int d = 1; d < 32; d <<= 1) { const uint32_t x = (uint32_t)__shfl_up((int)incl2, d, 32); if ((int)l >= d) incl2 += x; }
  const uint32_t excl = incl2 - sum;
  const uint32_t rel = (uint32_t)(need - acc0);                          // >= 1
  const uint32_t hm = (uint32_t)(__ballot(incl2 >= rel) >> hs);
  if (!hm) { o.e = p0 + 256 < N ? p0 + 256 : N; return o; }             // not reached (tables inconsistent): unclean
  const int fl = __builtin_ctz(hm);
  int tt = 8; uint32_t accv = 0, cv = 0;
#pragma unroll
  for (int t = 7; t >= 0; t--) if (excl + cs[t] >= rel) { tt = t; accv = excl + cs[t]; cv = b[t]; }
  tt = __shfl(tt, fl, 32); accv = (uint32_t)__shfl((int)accv, fl, 32); cv = (uint32_t)__shfl((int)cv, fl, 32);
  const uint64_t pe = p0 + 8u * (uint32_t)fl + (uint32_t)tt;
  o.e = pe + 1;
  bool next_fresh = pe + 1 >= N || in[pe + 1] != (uint8_t)cv;
  if (!next_fresh) {
    // the next block starts inside a run -- but a run of at most three bytes is all literals under either chunking (the one
    // counted from the run start and the one that starts afresh with the block), so the boundaries behind it are where the
    // speculation expects them: as good as a block start on a run boundary.  (text: "ll", "ee" at a block end)
    const uint8_t b = (uint8_t)cv;
    const uint32_t left = (pe >= 1 && in[pe - 1] == b) ? ((pe >= 2 && in[pe - 2] == b) ? 2u : 1u) : 0u;
    const uint32_t right = 1u + ((pe + 2 < N && in[pe + 2] == b) ? ((pe + 3 < N && in[pe + 3] == b) ? 2u : 1u) : 0u);
    next_fresh = 1u + left + right <= 3u;
  }
  o.clean = (accv == rel) && next_fresh;
  return o;
}

constexpr uint32_t NSPEC = 32;        // boundaries speculated per round: one 32-lane group each
__device__ uint64_t g_walk_dbg[8];     // CJS_DEBUG: [0] speculative rounds [1] serial steps [2],[3] their 100 MHz ticks
__global__ __launch_bounds__(1024) void rle_walk(const uint8_t* __restrict__ in, uint64_t N, uint32_t cap, uint32_t Tn,
                                                 const uint64_t* __restrict__ run_start_in, const uint64_t* __restrict__ next_bnd,
                                                 const uint64_t* __restrict__ gt, const uint16_t* __restrict__ subpre, const uint8_t* __restrict__ dmod,
                                                 RleBlock* __restrict__ blocks, uint32_t max_blocks, uint32_t* __restrict__ nblocks_out) {
  __shared__ uint32_t smem[1024 + 16];
  __shared__ unsigned long long sh64[2];
  __shared__ unsigned long long spec_e[NSPEC];
  __shared__ uint32_t spec_first_bad;
  uint64_t s = 0;
  uint32_t k = 0;
  bool done = false;
  uint64_t dbg_n[2] = {0, 0}, dbg_t[2] = {0, 0}, dbg_p[3] = {0, 0, 0};
  while (s < N && k < max_blocks && !done) {
    const uint64_t t_in = wall_clock64();
    // A round starts at s.  If s is a run boundary, fresh chunking == global chunking from s on and boundary j is where
    // G reaches G(s) + (j+1)*cap.  If s lies inside a run, only that run is chunked differently: with r_end its end and
    // base = bytes it emits under fresh chunking, the same holds with G(s) replaced by G(r_end) - base - unless the
    // block fills up inside the run or the run reaches the end of the input (closed forms below).
    uint64_t G0, r_end0 = s, Gr0; uint32_t base0 = 0;
    if (s == 0 || in[s] != in[s - 1]) {
      // G(s): tile prefix + in-tile prefix (one cooperative tile evaluation)
      const uint32_t t0 = (uint32_t)(s / RT);
      uint64_t fp; uint32_t below;
      walk_tile_eval(in, N, (uint64_t)t0 * RT, run_start_in[t0], 0, NONE64, s, smem, sh64, fp, below);
      G0 = gt[t0] + below; Gr0 = G0;
    } else {
      // end of the run containing s
      const uint32_t ts = (uint32_t)(s / RT);
      const uint64_t tile_end = ((uint64_t)(ts + 1) * RT < N) ? (uint64_t)(ts + 1) * RT : N;
      if (threadIdx.x == 0) sh64[0] = NONE64;
      __syncthreads();
      {
        unsigned long long mine = NONE64;
        for (int j = 0; j < 4; j++) {
          const uint64_t p = (uint64_t)ts * RT + (uint64_t)threadIdx.x * 4 + j;
          if (p > s && p < tile_end && mine == NONE64 && in[p] != in[p - 1]) mine = p;
        }
        if (mine != NONE64) atomicMin(&sh64[0], mine);
      }
      __syncthreads();
      uint64_t r_end = sh64[0];
      __syncthreads();
      if (r_end == NONE64) r_end = next_bnd[ts];
      const uint64_t g64 = emitted_fresh(r_end - s);
      if (g64 >= cap || r_end >= N) {
        uint64_t e; uint32_t len, base;
        if (g64 >= cap) { e = s + run_fill_input(cap); len = cap; base = cap; }     // the block fills up inside this run
        else { base = (uint32_t)g64; e = N; len = base; }                           // the run is the tail of the input
        if (threadIdx.x == 0) {
          RleBlock bd; bd.s = s; bd.e = e; bd.r_end = r_end; bd.Gr = 0; bd.len = len; bd.base = base;
          blocks[k] = bd;
        }
        k++;
        s = e;
        dbg_n[1]++; dbg_t[1] += wall_clock64() - t_in;
        if (len < cap) break;
        continue;
      }
      base0 = (uint32_t)g64; r_end0 = r_end;
      const uint32_t tr = (uint32_t)(r_end / RT);
      uint64_t fp; uint32_t below;
      walk_tile_eval(in, N, (uint64_t)tr * RT, run_start_in[tr], 0, NONE64, r_end, smem, sh64, fp, below);
      Gr0 = gt[tr] + below;
      G0 = Gr0 - base0;                         // >= one block's worth of emitted bytes: s > 0 here
    }
    {
      const uint64_t t_a = wall_clock64(); dbg_p[0] += t_a - t_in;
      const uint32_t j = threadIdx.x >> 5;               // group = speculated boundary
      if (threadIdx.x == 0) spec_first_bad = NSPEC;
      __syncthreads();
      SpecOut so = spec_boundary_group(in, N, Tn, gt, subpre, dmod, G0 + (uint64_t)(j + 1) * cap, G0 + (uint64_t)j * cap);
      const bool lead = (threadIdx.x & 31u) == 0;
      if (lead) spec_e[j] = so.e;
      const uint64_t t_b = wall_clock64(); dbg_p[1] += t_b - t_a;
      if (lead && (!so.clean || so.eof)) atomicMin(&spec_first_bad, j);
      __syncthreads();
      dbg_p[2] += wall_clock64() - t_b;
      const uint32_t m = spec_first_bad;                    // boundaries 0..m-1 are clean; boundary m is EOF or unclean
      // blocks k+j for j <= m (block j spans (boundary j-1, boundary j]); the one ending at boundary m is still exact
      if (lead && j <= m && k + j < max_blocks) {
        const uint64_t bs = j == 0 ? s : spec_e[j - 1];
        RleBlock bd; bd.s = bs; bd.r_end = bs; bd.base = 0; bd.Gr = G0 + (uint64_t)j * cap;
        if (j == 0) { bd.r_end = r_end0; bd.base = base0; bd.Gr = Gr0; }
        bool emit = true;
        if (so.eof) { bd.e = N; bd.len = so.len_last; emit = so.len_last > 0 && bs < N; }
        else { bd.e = so.e; bd.len = cap; }
        if (j < m || (j == m && m < NSPEC)) { if (emit) blocks[k + j] = bd; }
      }
      __syncthreads();
      // advance: count emitted blocks
      if (m < NSPEC) {
        // boundary m: EOF (stream ends) or unclean (the next round starts inside a run)
        const unsigned long long e_m = spec_e[m];
        // was block m emitted?  eof with zero length -> not
        const uint64_t tgt_prev = G0 + (uint64_t)m * cap;
        const bool eof_m = gt[Tn] < tgt_prev + cap;
        if (eof_m) { const bool has = gt[Tn] > tgt_prev && (m == 0 ? s : spec_e[m - 1]) < N; k += m + (has ? 1u : 0u); done = true; }
        else { k += m + 1; s = e_m; }
      } else { k += NSPEC; s = spec_e[NSPEC - 1]; }
      __syncthreads();
      dbg_n[0]++; dbg_t[0] += wall_clock64() - t_in;
    }
  }
  if (threadIdx.x == 0) { *nblocks_out = k; g_walk_dbg[0] = dbg_n[0]; g_walk_dbg[1] = dbg_n[1]; g_walk_dbg[2] = dbg_t[0]; g_walk_dbg[3] = dbg_t[1]; g_walk_dbg[4] = dbg_p[0]; g_walk_dbg[5] = dbg_p[1]; g_walk_dbg[6] = dbg_p[2]; }
}


// ---- multi-GPU jobs: a rank makes the tile tables of ITS share of the tiles only (tiles [t0, t1)).  What the tile scans
// would have carried in from the other tiles is found by looking at the input itself (every rank holds the stream): the last
// run boundary in front of tile t0 and the first one at or behind tile t1 -- nearly always inside the neighbouring tile; a
// giant run makes the probe walk on, 16 KiB per step.  carry[0] = (last boundary position) + 1 or 0, carry[1] = first
// boundary position or N (see rle_scanb_apply).  One workgroup.
__global__ __launch_bounds__(1024) void rle_probe(const uint8_t* __restrict__ in, uint64_t N, uint32_t t0, uint32_t t1, uint64_t* __restrict__ carry) {
  __shared__ unsigned long long sm[16];
  const uint64_t lo = (uint64_t)t0 * RT, hi = (uint64_t)t1 * RT < N ? (uint64_t)t1 * RT : N;
  unsigned long long back = 0;
  for (uint64_t wend = lo; wend > 0 && !back;) {                      // windows [wend - 16 KiB, wend), walking towards 0
    const uint64_t wbeg = wend > 16384 ? wend - 16384 : 0;
    const uint64_t p0 = wbeg + (uint64_t)threadIdx.x * 16;
    unsigned long long mine = 0;
    if (p0 < wend) {
      uint8_t b[16];
      uint32_t last;
      if (boundaries16(in, N, p0, wend, b, last)) mine = p0 + last;          // (my last boundary) + 1
    }
    back = block_incl_max<1024>(mine, sm);
    __syncthreads();
    if (threadIdx.x == 1023) sm[0] = back;
    __syncthreads();
    back = sm[0];
    __syncthreads();
    wend = wbeg;
  }
  unsigned long long fwd = N;
  for (uint64_t wbeg = hi; wbeg < N && fwd == N; wbeg += 16384) {
    const uint64_t p0 = wbeg + (uint64_t)threadIdx.x * 16;
    unsigned long long mine = 0;                                      // NONE64 - position of the first boundary, 0 = none
    if (p0 < N) {
      uint8_t b[16];
      uint32_t last;
      const uint32_t bm = boundaries16(in, N, p0, N, b, last);
      if (bm) mine = NONE64 - (p0 + (uint32_t)__builtin_ctz(bm));
    }
    const unsigned long long m = block_incl_max<1024>(mine, sm);
    __syncthreads();
    if (threadIdx.x == 1023) sm[0] = m;
    __syncthreads();
    if (sm[0]) fwd = NONE64 - sm[0];
    __syncthreads();
  }
  if (threadIdx.x == 0) { carry[0] = back; carry[1] = fwd; }
}
// the whole stream's tile tables from the ranks' shares, gathered back to back (share r = tiles [r*tpr, (r+1)*tpr) in the layout
// of Rle1Work::tile_share): one thread per tile
__global__ __launch_bounds__(256) void rle_tables_unpack(const uint8_t* __restrict__ recv, uint32_t tpr, uint32_t Tn, uint64_t* __restrict__ fb, uint64_t* __restrict__ lb,
                                                         uint64_t* __restrict__ gt, uint16_t* __restrict__ subpre, uint8_t* __restrict__ dmod) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= Tn) return;
  const uint32_t r = t / tpr, j = t - r * tpr;
  const TileShare L = tile_share(tpr);
  const uint8_t* base = recv + (size_t)r * L.bytes;
  lb[t] = reinterpret_cast<const uint64_t*>(base + L.lb)[j];
  fb[t] = reinterpret_cast<const uint64_t*>(base + L.fb)[j];
  gt[t] = reinterpret_cast<const uint64_t*>(base + L.gt)[j];
  const uint4* sp = reinterpret_cast<const uint4*>(base + L.subpre) + (size_t)2 * j;
  uint4* dp = reinterpret_cast<uint4*>(subpre + (size_t)t * 16);
  dp[0] = sp[0]; dp[1] = sp[1];
  reinterpret_cast<uint4*>(dmod + (size_t)t * 16)[0] = (reinterpret_cast<const uint4*>(base + L.dmod))[j];
}

__global__ void rle_block_lens(const RleBlock* __restrict__ blocks, uint32_t* nblocks_p, uint32_t* __restrict__ block_len) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x, nb = nblocks_p[0];
  if (k < nb) block_len[k] = blocks[k].len;
  if (k + 1 == nb) nblocks_p[1] = blocks[k].len;      // length of the last block: goes to the host with the count
}

// ------------------------------------------------------------------------------------------
size_t Rle1Work::bytes_needed(size_t max_in, uint32_t cap, size_t range_blocks) {
  const size_t Tn = (max_in + RT - 1) / RT + 2;
  const size_t maxb = max_blocks_for(max_in, cap);
  const size_t segs = max_segs_for(cap);
  size_t b = 0;
  auto add = [&](size_t n) { b += (n + 255) & ~(size_t)255; };
  add(Tn * 8); add(Tn * 8); add((Tn + 1) * 8); add(Tn * 16 * 2); add(Tn * 16); add(3 * (Tn / 1024 + 2) * 8);
  add(maxb * sizeof(RleBlock)); add(maxb * 4); add(maxb * 4); add(64);
  add((range_blocks ? range_blocks : maxb) * segs * 4);
  return b + 4096;
}
int Rle1Work::carve(Arena& a, size_t max_in_, uint32_t cap_, size_t range_blocks_) {
  max_in = max_in_; cap = cap_;
  const size_t Tn = (max_in + RT - 1) / RT + 2;
  max_blocks = (uint32_t)max_blocks_for(max_in, cap);
  max_segs = (uint32_t)max_segs_for(cap);
  fb = a.take<uint64_t>(Tn); lb = a.take<uint64_t>(Tn); gt = a.take<uint64_t>(Tn + 1);
  agg = a.take<unsigned long long>(3 * (Tn / 1024 + 2));
  subpre = a.take<uint16_t>(Tn * 16); dmod = a.take<uint8_t>(Tn * 16);
  blocks = a.take<RleBlock>(max_blocks); block_len = a.take<uint32_t>(max_blocks); block_crc = a.take<uint32_t>(max_blocks);
  nblocks = a.take<uint32_t>(16);
  range_blocks = (uint32_t)(range_blocks_ ? range_blocks_ : max_blocks);
  seg_crc = a.take<uint32_t>((size_t)range_blocks * max_segs);
  return seg_crc ? 0 : CJS_E_OUT_OF_MEMORY;
}

// Stage 0a, first half: the tile tables (run start carried into each tile, next boundary behind it, emitted bytes under the
// global chunking, subtile tables) of tiles [t0, t1) of d_in[0..N).  `share` null: into the workspace's own arrays (absolute
// tile index); else into a share buffer of Rle1Work::share_bytes(tpr) bytes that a multi-GPU job exchanges (tile t0 first).
int rle1_tiles(hipStream_t s, Rle1Work& w, const uint8_t* d_in, uint64_t N, uint32_t t0, uint32_t t1, uint8_t* share, uint32_t tpr) {
  if (N > w.max_in) return CJS_E_INVALID_ARG;
  const uint32_t Tn = tiles_for(N);
  if (t1 > Tn) t1 = Tn;
  if (t0 >= t1) return 0;
  uint64_t *fb = w.fb, *lb = w.lb, *gt = w.gt; uint16_t* subpre = w.subpre; uint8_t* dmod = w.dmod;
  if (share) {                                       // kernels index by absolute tile: tile t0 is entry 0 of the share
    if (t1 - t0 > tpr) return CJS_E_INVALID_ARG;
    const TileShare L = tile_share(tpr);
    lb = reinterpret_cast<uint64_t*>(share + L.lb) - t0; fb = reinterpret_cast<uint64_t*>(share + L.fb) - t0;
    gt = reinterpret_cast<uint64_t*>(share + L.gt) - t0;
    subpre = reinterpret_cast<uint16_t*>(share + L.subpre) - (size_t)t0 * 16; dmod = share + L.dmod - (size_t)t0 * 16;
  }
  const uint32_t Tl = t1 - t0, nch = (Tl + SC - 1) / SC;
  uint64_t* carry = reinterpret_cast<uint64_t*>(w.nblocks + 4);      // two u64 behind the block count
  hipLaunchKernelGGL(rle_tile_summary, dim3(Tl), dim3(256), 0, s, d_in, N, fb, lb, t0);
  hipLaunchKernelGGL(rle_probe, dim3(1), dim3(1024), 0, s, d_in, N, t0, t1, carry);
  hipLaunchKernelGGL(rle_scanb_reduce, dim3(nch), dim3(1024), 0, s, fb + t0, lb + t0, Tl, w.agg, nch);
  hipLaunchKernelGGL(rle_scanb_mid, dim3(1), dim3(1024), 0, s, w.agg, nch);
  hipLaunchKernelGGL(rle_scanb_apply, dim3(nch), dim3(1024), 0, s, fb + t0, lb + t0, Tl, w.agg, nch, carry);
  hipLaunchKernelGGL(rle_tile_count, dim3(Tl), dim3(256), 0, s, d_in, N, lb, gt, subpre, dmod, t0);
  CJS_HIP_TRY(hipGetLastError());
  return 0;
}
// the gathered shares of all ranks (rank-major, share r = tiles [r*tpr, (r+1)*tpr)) -> the workspace's arrays
int rle1_tables_from_shares(hipStream_t s, Rle1Work& w, uint64_t N, const uint8_t* d_recv, uint32_t tpr) {
  const uint32_t Tn = tiles_for(N);
  if (!Tn) return 0;
  hipLaunchKernelGGL(rle_tables_unpack, dim3((Tn + 255) / 256), dim3(256), 0, s, d_recv, tpr, Tn, w.fb, w.lb, w.gt, w.subpre, w.dmod);
  CJS_HIP_TRY(hipGetLastError());
  return 0;
}
// Stage 0a, second half: prefix of the emitted bytes over the tiles and the boundary walk.  Leaves descriptors / lengths on the
// device, returns the number of blocks in *nblocks_host (syncs the stream).
int rle1_walk_run(hipStream_t s, Rle1Work& w, const uint8_t* d_in, uint64_t N, uint32_t* nblocks_host, uint32_t* last_len_host) {
  if (N > w.max_in) return CJS_E_INVALID_ARG;
  if (N == 0) { *nblocks_host = 0; if (last_len_host) *last_len_host = 0; CJS_HIP_TRY(hipMemsetAsync(w.nblocks, 0, 4, s)); return 0; }
  const uint32_t Tn = tiles_for(N);
  const uint32_t nch = (Tn + SC - 1) / SC;
  hipLaunchKernelGGL(rle_scanc_reduce, dim3(nch), dim3(1024), 0, s, w.gt, Tn, w.agg, nch);
  hipLaunchKernelGGL(rle_scanc_mid, dim3(1), dim3(1024), 0, s, w.agg, nch, w.gt, Tn);
  hipLaunchKernelGGL(rle_scanc_apply, dim3(nch), dim3(1024), 0, s, w.gt, Tn, w.agg, nch);
  hipLaunchKernelGGL(rle_walk, dim3(1), dim3(1024), 0, s, d_in, N, w.cap, Tn, w.lb, w.fb, w.gt, w.subpre, w.dmod, w.blocks, w.max_blocks, w.nblocks);
  hipLaunchKernelGGL(rle_block_lens, dim3((w.max_blocks + 255) / 256), dim3(256), 0, s, w.blocks, w.nblocks, w.block_len);
  CJS_HIP_TRY(hipGetLastError());
  if (!w.h_n) CJS_HIP_TRY(hipHostMalloc((void**)w.h_n.put(), 16));
  CJS_HIP_TRY(hipMemcpyAsync(w.h_n, w.nblocks, 8, hipMemcpyDeviceToHost, s));
  CJS_HIP_TRY(hipStreamSynchronize(s));
  *nblocks_host = w.h_n[0];
  if (last_len_host) *last_len_host = w.h_n[0] ? w.h_n[1] : 0u;
  if (env_debug()) {
    uint64_t d[8];
    if (hipMemcpyFromSymbol(d, HIP_SYMBOL(g_walk_dbg), sizeof d) == hipSuccess)
      fprintf(stderr, "[cjs rle] boundary walk: %llu speculative rounds %.1f us, %llu serial steps %.1f us, %u blocks; thread 0 of the rounds: tile eval %.1f us, own search %.1f us, wait for the slowest lane %.1f us\n", (unsigned long long)d[0], d[2] / 100.0,
              (unsigned long long)d[1], d[3] / 100.0, w.h_n[0], d[4] / 100.0, d[5] / 100.0, d[6] / 100.0);
  }
  return 0;
}
// Stage 0a: block boundaries of the whole stream d_in[0..N) on one GPU
int rle1_run(hipStream_t s, Rle1Work& w, const uint8_t* d_in, uint64_t N, uint32_t* nblocks_host, uint32_t* last_len_host) {
  if (N > w.max_in) return CJS_E_INVALID_ARG;
  if (N) CJS_TRY(rle1_tiles(s, w, d_in, N, 0u, tiles_for(N), nullptr, 0u));
  return rle1_walk_run(s, w, d_in, N, nblocks_host, last_len_host);
}
}  // namespace cjs
