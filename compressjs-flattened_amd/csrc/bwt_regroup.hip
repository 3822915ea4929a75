// bwt_regroup.hip — the regroup behind every sort of the suffix sort (the map: bwt.hip): per-tile counts, their scan, bwt_apply;
// the keys and flag bytes of the whole-array fallbacks; and the emit passes at the end of a run.
#include "bwt_dev.hpp"

namespace cjs {

// Two-sweep scheduling of the round-1 rank scatter: a block's 3.6 MB rank region does not survive in a 4 MiB L2 next to
// the streamed arrays (PMC: ~64 B of memory traffic per 4-byte store), so the tiles are walked twice, storing first the ranks
// of the lower half of every block's text positions, then the upper half (1.8 MB per sweep and block; the tiles of a block
// stay on one XCD, see xcd_tile).
// PMC: WRITE_SIZE of the kernel 6.66 -> 2.67 GB per 100 MB step; its time 1.64 -> 1.35 ms (the second sweep re-reads and
// re-derives the group structure).  The same scheduling applied to the gather / scatter of rounds >= 2 over the compacted
// arrays (per-block start table from a binary search) was measured SLOWER (gather 0.84 -> 1.07 ms, scatter 1.24 -> 1.84 ms
// in round 2) and is not kept.
struct HalfMap { uint32_t halves, stride; };      // halves 2: the two sweeps are the launches SWEEP 1 and SWEEP 2 of bwt_apply

// Heads per 4096-slot tile of the head bytes, and their exclusive sums in place: the group ordinals of bwt_gather_keys when the
// array spans more than two tiles (the overflow fallback; rare, not tuned)
__global__ __launch_bounds__(256) void bwt_head_counts(const uint8_t* __restrict__ ghead, uint32_t A, uint32_t* __restrict__ tsum) {
  __shared__ uint32_t sm[4];
  const uint64_t base = (uint64_t)blockIdx.x * RS_TILE;
  const uint32_t nvalid = (uint32_t)((uint64_t)A - base < RS_TILE ? (uint64_t)A - base : RS_TILE);
  uint32_t valid;
  const uint4 v = hf_load16(ghead, base, nvalid, threadIdx.x, valid);
  const uint32_t n = block_sum<256>((uint32_t)__popc(hf_bits16(v, 0) & valid), sm);
  if (threadIdx.x == 0) tsum[blockIdx.x] = n;
}
__global__ __launch_bounds__(1024) void bwt_head_scan(uint32_t* __restrict__ tsum, uint32_t T) {
  __shared__ uint32_t sm[16];
  uint32_t carry = 0;
  for (uint32_t base = 0; base < T; base += 1024) {
    const uint32_t i = base + threadIdx.x;
    uint32_t tot;
    const uint32_t ex = block_excl_sum<1024>(i < T ? tsum[i] : 0u, sm, tot);
    if (i < T) tsum[i] = carry + ex;
    carry += tot;
  }
}
// keys of a round >= 2 for the whole-array sorts: (group ordinal, rank of suffix i+h).  The ordinal of a slot is the number of
// heads up to and including it, less one: heads in front of the tile from tsum, or (tsum null, at most two tiles: the small
// rounds) counted by the workgroup itself; inside the tile from the head bytes as 64 mask words.
template <typename G>
__global__ __launch_bounds__(256) void bwt_gather_keys(G g, int cyclic, uint32_t A, uint32_t h, const uint32_t* __restrict__ R,
                                                       const uint32_t* __restrict__ val, const uint32_t* __restrict__ pos,
                                                       const uint8_t* __restrict__ ghead, const uint32_t* __restrict__ tsum, uint64_t* __restrict__ key, uint32_t T) {
  __shared__ uint64_t m_h[64];
  __shared__ uint32_t wp_h[64];
  __shared__ uint32_t sm[4];
  const uint32_t tile = xcd_tile(blockIdx.x, T);
  if (tile >= T) return;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const uint64_t base = (uint64_t)tile * RS_TILE;
  const uint32_t nvalid = (uint32_t)((uint64_t)A - base < RS_TILE ? (uint64_t)A - base : RS_TILE);
  // three batches of sixteen independent loads each (streams, then the rank gathers, then the stores): as one loop the
  // compiler waits for every gather before it issues the next
  uint32_t p16[16], v16[16], kk[16];
  uint32_t hvalid;
  const uint4 hv = hf_load16(ghead, base, nvalid, tid, hvalid);
#pragma unroll
  for (int it = 0; it < 16; it++) {
    const uint32_t e = (uint32_t)it * 256 + threadIdx.x;
    const uint64_t a = base + (e < nvalid ? e : nvalid - 1u);
    p16[it] = __builtin_nontemporal_load(pos + a); v16[it] = __builtin_nontemporal_load(val + a);
  }
  uint32_t obase = tsum ? tsum[tile] : 0u;      // heads in front of the tile
  if (!tsum) for (uint32_t t = 0; t < tile; t++) {
    uint32_t pvalid;
    const uint4 pvv = hf_load16(ghead, (uint64_t)t * RS_TILE, RS_TILE, tid, pvalid);
    obase += block_sum<256>((uint32_t)__popc(hf_bits16(pvv, 0)), sm);
  }
  reinterpret_cast<uint16_t*>(m_h)[tid] = (uint16_t)(hf_bits16(hv, 0) & hvalid);
  __syncthreads();
  if (w == 0) { const uint32_t n = (uint32_t)__popcll(m_h[lane]); wp_h[lane] = wave_incl_sum(n) - n; }
  __syncthreads();
  uint32_t blk = p16[0] / g.stride;             // (pos[] ascends along the array: blk_step)
#pragma unroll
  for (int it = 0; it < 16; it++) {
    blk = blk_step(p16[it], g.stride, blk);
    const uint32_t n = blk_len(g, blk);
    uint32_t j = pk_pos(v16[it]) + h;// (both below 2^31; the top byte of val[] may carry the byte in front of the suffix)
    if (cyclic) { if (j >= n) j %= n; }
    const bool past = !cyclic && j >= n;
    kk[it] = R[(size_t)blk * g.stride + (past ? 0 : j)] + 1u;
    if (past) kk[it] = 0u;
  }
#pragma unroll
  for (int it = 0; it < 16; it++) {
    const uint32_t e = (uint32_t)it * 256 + threadIdx.x;
    const int wi = it * 4 + w;                  // slot e = 64 * wi + lane
    const uint32_t ord = obase + wp_h[wi] + (uint32_t)__popcll(m_h[wi] & mask_le(lane)) - 1u;      // (slot 0 of the array is a head)
    if (e < nvalid) __builtin_nontemporal_store(round_key(ord, kk[it]), key + base + e);
  }
}

// What the regroup counts per 4096-tile, for bwt_scan_tiles: #surviving elements, #surviving group heads, (last new-head index)+1.
// Three kernels count them (bwt_flags, bwt_flags_bytes, sweep 1 of bwt_apply), each with the large-group test (run_without_head).
__device__ __forceinline__ void store_tile_counts(uint32_t* __restrict__ tile_cnt, uint32_t T, uint32_t tile, uint32_t surv, uint32_t heads, uint32_t last) {
  tile_cnt[tile] = surv; tile_cnt[T + tile] = heads; tile_cnt[2 * (size_t)T + tile] = last;
}
// ... from the partial counts of the 256 threads of workgroup = tile (last: their maximum); sm: 4 words
__device__ __forceinline__ void reduce_tile_counts(uint32_t surv, uint32_t heads, uint32_t last, uint32_t* sm, uint32_t* __restrict__ tile_cnt, uint32_t T) {
  surv = block_sum<256>(surv, sm);
  heads = block_sum<256>(heads, sm);
  last = wave_max(last);
  if (lane_id() == 0) sm[wave_id()] = last;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t m = sm[0]; for (int i = 1; i < 4; i++) m = sm[i] > m ? sm[i] : m;
    store_tile_counts(tile_cnt, T, blockIdx.x, surv, heads, m);
  }
}

__global__ __launch_bounds__(256) void bwt_flags(const uint64_t* __restrict__ key, uint32_t A, uint32_t* __restrict__ tile_cnt, uint32_t T, int gshift,
                                                 uint32_t* __restrict__ big_flag, uint32_t first_stride /* round 1: block stride (a block start is a head), else 0 */) {
  __shared__ uint64_t sk[RS_TILE + 2];
  __shared__ uint32_t sm[4];
  __shared__ uint32_t hword[64];          // per 64-slot word: holds a new group head
  const uint64_t base = (uint64_t)blockIdx.x * RS_TILE;
  const uint32_t nvalid = (uint32_t)((uint64_t)A - base < RS_TILE ? (uint64_t)A - base : RS_TILE);
  uint32_t surv = 0, heads = 0, last = 0;
  const uint64_t bnd = first_stride ? (base + first_stride - 1u) / first_stride * first_stride : ~0ull;      // the block start in [base, base + tile]
  // the tile's keys go through LDS so that every global load is issued up front (neighbours come from LDS, not from three
  // loads per element that the compiler waits for one by one)
  uint64_t k[16];
#pragma unroll
  for (int it = 0; it < 16; it++) {
    const uint32_t loc = (uint32_t)it * 256 + threadIdx.x;
    k[it] = key[base + (loc < nvalid ? loc : nvalid - 1u)] >> gshift;            // packed round-1 records: the low bits are the position
  }
  if (threadIdx.x == 0) sk[0] = base ? key[base - 1] >> gshift : 0;
  if (threadIdx.x == 64) sk[RS_TILE + 1] = base + RS_TILE < A ? key[base + RS_TILE] >> gshift : 0;
#pragma unroll
  for (int it = 0; it < 16; it++) sk[1u + (uint32_t)it * 256 + threadIdx.x] = k[it];
  __syncthreads();
#pragma unroll
  for (int it = 0; it < 16; it++) {
    const uint32_t loc = (uint32_t)it * 256 + threadIdx.x;
    const uint64_t a = base + loc;
    if (loc < nvalid) {
      const bool nh = a == 0 || a == bnd || sk[loc] != k[it];
      const bool nx = a + 1 == A || a + 1 == bnd || sk[loc + 2] != k[it];
      const bool single = nh && nx;
      surv += !single;
      heads += nh && !single;
      if (nh) last = (uint32_t)a + 1u;
    }
    const uint64_t hb = __ballot(loc < nvalid && (base + loc == 0 || base + loc == bnd || sk[loc] != k[it]));
    if (lane_id() == 0) hword[it * 4 + wave_id()] = hb != 0;
  }
  __syncthreads();
  if (wave_id() == 0) {                   // the large-group test: eight words to a run
    const uint64_t nz = __ballot(hword[lane_id()] != 0);
    if (run_without_head(nz, 8, base, A) && lane_id() == 0) atomicOr(big_flag, 1u);
  }
  reduce_tile_counts(surv, heads, last, sm, tile_cnt, T);
}

// Rounds >= 2: the sorters leave one flag byte per slot instead of a 64-bit key -- all that the regroup ever took out of the key.
// A slot has exactly one writer per round (the window that owns its group, else bwt_defer_scatter, else bwt_key_flags).
// sorted 64-bit keys (group ordinal << 20 | rank key) -> flag bytes: the whole-array fallbacks of a round >= 2
__global__ __launch_bounds__(256) void bwt_key_flags(const uint64_t* __restrict__ key, uint32_t A, uint8_t* __restrict__ hflag) {
  for (uint64_t a = (uint64_t)blockIdx.x * 256 + threadIdx.x; a < A; a += (uint64_t)gridDim.x * 256) {
    const uint64_t k = key[a], p = a ? key[a - 1] : ~k;
    hflag[a] = hf_of_sorted(k, p);
  }
}
// bwt_flags of a round >= 2, from the flag bytes: 1 B per slot
__global__ __launch_bounds__(256) void bwt_flags_bytes(const uint8_t* __restrict__ hflag, uint32_t A, uint32_t* __restrict__ tile_cnt, uint32_t T,
                                                       uint32_t* __restrict__ big_flag) {
  __shared__ uint32_t nhs[257];           // per thread: new-head mask of its 16 slots (slots at or past A count as heads)
  __shared__ uint32_t sm[4];
  const int tid = threadIdx.x;
  const uint64_t base = (uint64_t)blockIdx.x * RS_TILE;
  const uint32_t nvalid = (uint32_t)((uint64_t)A - base < RS_TILE ? (uint64_t)A - base : RS_TILE);
  uint32_t valid;
  const uint4 v = hf_load16(hflag, base, nvalid, tid, valid);
  const uint32_t nh = hf_bits16(v, 0) & valid;
  nhs[tid] = nh | (~valid & 0xFFFFu);
  if (tid == 0) nhs[256] = base + RS_TILE < A ? (uint32_t)hflag[base + RS_TILE] & HF_NEW : 1u;
  __syncthreads();
  const uint32_t nx = ((nhs[tid] >> 1) | (nhs[tid + 1] << 15)) & 0xFFFFu;      // the slot behind is a head (or the end of the array)
  const uint32_t single = nh & nx;
  uint32_t surv = (uint32_t)__popc(valid & ~single), heads = (uint32_t)__popc(nh & ~single);
  uint32_t last = nh ? (uint32_t)base + (uint32_t)tid * 16u + 32u - (uint32_t)__clz(nh) : 0u;
  {                                       // the large-group test: a wave holds two runs, 32 threads of 16 slots to a run
    const uint64_t any = __ballot(nh != 0);
    if (run_without_head(any, 32, base + (uint64_t)wave_id() * (2u * LG_RUN), A) && lane_id() == 0) atomicOr(big_flag, 1u);
  }
  reduce_tile_counts(surv, heads, last, sm, tile_cnt, T);
}

// single workgroup: exclusive sums of [0],[1]; exclusive prefix-max of [2]; totals -> counters[0..1]
// (eight consecutive tiles per thread, one round of workgroup scans per 8 K tiles: 78 instead of 44 us for the 24 K tiles of
// round 1 -- the strided accesses cost more than the barriers saved)
__global__ __launch_bounds__(1024) void bwt_scan_tiles(uint32_t* __restrict__ tile_cnt, uint32_t T, uint32_t* __restrict__ counters,
                                                      uint32_t* __restrict__ host_mirror /* pinned host memory, read after the stream sync */) {
  __shared__ uint32_t sm[16];
  __shared__ uint32_t mx[1024];
  uint32_t c0 = 0, c1 = 0, cm = 0;
  for (uint32_t base = 0; base < T; base += 1024) {
    const uint32_t i = base + threadIdx.x;
    const bool ok = i < T;
    uint32_t t0, t1;
    const uint32_t v0 = ok ? tile_cnt[i] : 0u, v1 = ok ? tile_cnt[T + i] : 0u, v2 = ok ? tile_cnt[2 * (size_t)T + i] : 0u;
    const uint32_t e0 = block_excl_sum<1024>(v0, sm, t0);
    const uint32_t e1 = block_excl_sum<1024>(v1, sm, t1);
    const uint32_t im = block_incl_max<1024>(v2, sm);
    mx[threadIdx.x] = im;
    __syncthreads();
    const uint32_t prev = threadIdx.x ? mx[threadIdx.x - 1] : 0u;
    const uint32_t chunk_max = mx[1023];
    __syncthreads();
    if (ok) {
      tile_cnt[i] = c0 + e0; tile_cnt[T + i] = c1 + e1;
      tile_cnt[2 * (size_t)T + i] = prev > cm ? prev : cm;
    }
    c0 += t0; c1 += t1; cm = chunk_max > cm ? chunk_max : cm;
  }
  if (threadIdx.x == 0) {      // (CN_LARGE_GROUP: a group may exceed 1023 slots, from the three counting kernels)
    counters[CN_SURVIVORS] = c0; counters[CN_GROUPS] = c1; host_mirror[CN_SURVIVORS] = c0; host_mirror[CN_GROUPS] = c1;
    host_mirror[CN_LARGE_GROUP] = counters[CN_LARGE_GROUP]; counters[CN_LARGE_GROUP] = 0;
  }
}

// regroup: new ranks -> R (scattered 4-byte stores), singletons -> SA, survivors compacted into the next
// active arrays.  Fully lane-striped: the per-element prefix quantities come from 4096-bit masks
// (wave ballots) + a 64-word scan, so every global access of a wave touches consecutive addresses.
// SWEEP 0: one launch behind a counting pass (bwt_flags + bwt_scan_tiles).
// SWEEP 1 / 2 (round 1, packed records; see HalfMap): two launches with the tile scan between them, and NO counting pass
// in front -- sweep 1 stores the ranks of the lower half-blocks and leaves the tile counts that bwt_flags would have made
// (it finds the one class head it cannot see by search: class_head_before); sweep 2 stores the upper half and, with the
// scanned counts, everything else.
template <bool FIRST, bool PACKED, int SWEEP = 0, typename G = Geom>      // FIRST: round 1 - slot a is sorted position a, and there is no previous grouping
__global__ __launch_bounds__(256) void bwt_apply(const uint64_t* __restrict__ key /* FIRST */, const uint8_t* __restrict__ hflag /* !FIRST: flag bytes instead */,
                                                 const uint32_t* __restrict__ val,
                                                 const uint32_t* __restrict__ pos, uint32_t A, G g,
                                                 uint32_t* tile_cnt, uint32_t T,
                                                 uint32_t* __restrict__ R, uint32_t* __restrict__ SA,
                                                 uint32_t* __restrict__ nval, uint32_t* __restrict__ npos, uint8_t* __restrict__ nhead /* per survivor: 1 = starts a group */, HalfMap hm_,
                                                 const uint8_t* __restrict__ Tx, uint8_t* __restrict__ U, uint32_t* __restrict__ big_flag,
                                                 int gs1 /* FIRST: group key = key >> gs1 */, int carried /* the byte in front of a suffix rides in its record / val */) {
  __shared__ uint64_t sk[FIRST ? RS_TILE + 2 : 1];        // rounds >= 2 stage no keys: 4 KB of LDS instead of 36
  __shared__ uint64_t m_nh[64], m_sg[64], m_oh[64];
  __shared__ uint32_t wp_s[64], wp_head[64];
  __shared__ uint32_t carry_s, nx_s;
  const uint32_t tile = xcd_tile(blockIdx.x, T), half = SWEEP == 2 ? 1u : 0u;
  if (tile >= T) return;
  const uint32_t hsplit = hm_.stride >> 1;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const uint64_t base = (uint64_t)tile * RS_TILE;
  const uint32_t nvalid = (uint32_t)((uint64_t)A - base < RS_TILE ? (uint64_t)A - base : RS_TILE);
  // every streaming load of the tile is issued up front (one loop of load + LDS store makes the compiler wait per load)
  uint32_t sbase = 0, carry = 0;
  if (SWEEP != 1) { sbase = tile_cnt[tile]; carry = tile_cnt[2 * (size_t)T + tile]; }
  else if (w == 0) {
    const uint64_t seg0 = (uint64_t)((uint32_t)base / g.stride) * g.stride;     // (round 1: slot = sorted position)
    const uint32_t c = (uint32_t)class_head_before(key, seg0, base, gs1, lane) + 1u;
    if (lane == 0) carry_s = c;
  }
  uint32_t p16[FIRST ? 1 : 16], v16[PACKED ? 1 : 16];
  {
    uint64_t k16[FIRST ? 16 : 1];
    uint4 hv = make_uint4(0u, 0u, 0u, 0u);
    uint32_t hvalid = 0;
    if constexpr (FIRST) {
#pragma unroll
      for (int it = 0; it < 16; it++) {
        const uint32_t e = (uint32_t)it * 256u + tid;
        k16[it] = __builtin_nontemporal_load(key + base + (e < nvalid ? e : nvalid - 1u));     // streamed once: keep the L2 for R
      }
    } else hv = hf_load16(hflag, base, nvalid, tid, hvalid);      // this thread's 16 slots are [16 * tid, +16): one load
    if (!FIRST) {
#pragma unroll
      for (int it = 0; it < 16; it++) { const uint32_t e = (uint32_t)it * 256u + tid; p16[it] = __builtin_nontemporal_load(pos + base + (e < nvalid ? e : nvalid - 1u)); }
    }
    if (!PACKED) {
#pragma unroll
      for (int it = 0; it < 16; it++) { const uint32_t e = (uint32_t)it * 256u + tid; v16[it] = __builtin_nontemporal_load(val + base + (e < nvalid ? e : nvalid - 1u)); }
    }
    if constexpr (FIRST) {
      if (tid == 0) sk[0] = base ? key[base - 1] : ~0ull;
      if (tid == 64) sk[RS_TILE + 1] = base + RS_TILE < A ? key[base + RS_TILE] : ~0ull;
#pragma unroll
      for (int it = 0; it < 16; it++) {
        const uint32_t e = (uint32_t)it * 256u + tid;
        sk[e + 1] = e < nvalid ? k16[it] : ~0ull;
      }
    } else {
      // the head masks are the flag bits themselves: 16 bits per thread, laid over the 64 mask words
      reinterpret_cast<uint16_t*>(m_nh)[tid] = (uint16_t)(hf_bits16(hv, 0) & hvalid);
      reinterpret_cast<uint16_t*>(m_oh)[tid] = (uint16_t)(hf_bits16(hv, 1) & hvalid);
      if (tid == 64) nx_s = base + RS_TILE < A ? (uint32_t)hflag[base + RS_TILE] & HF_NEW : 1u;      // the slot behind the tile is a head
    }
  }
  __syncthreads();
  if constexpr (FIRST) {
    const int GS = gs1;                          // packed records: the group key sits above the position (and carried byte) bits
    const uint64_t bnd = (base + g.stride - 1u) / g.stride * g.stride;      // round 1: a block start is a head (slot = sorted position)
#pragma unroll 4
    for (int it = 0; it < 16; it++) {
      const uint32_t e = (uint32_t)it * 256u + tid;
      const uint64_t a = base + e;
      const bool ok = e < nvalid;
      const uint64_t k = sk[e + 1] >> GS;
      const bool nh = ok && (a == 0 || a == bnd || (sk[e] >> GS) != k);
      const bool nx = a + 1 == A || a + 1 == bnd || (sk[e + 2] >> GS) != k;
      const uint64_t mnh = __ballot(nh), msg = __ballot(nh && nx);
      if (lane == 0) { m_nh[it * 4 + w] = mnh; m_sg[it * 4 + w] = msg; }
    }
    __syncthreads();
  }
  if (w == 0) {                          // 64 mask words, one per lane
    const uint64_t mh = m_nh[lane];
    const uint32_t first = (uint32_t)lane * 64u;
    const uint32_t nv = nvalid > first ? (nvalid - first < 64u ? nvalid - first : 64u) : 0u;
    const uint64_t vm = nv == 64 ? ~0ull : ((1ull << nv) - 1ull);
    uint64_t ms;
    if constexpr (FIRST) ms = m_sg[lane];
    else {                               // singleton = head whose next slot is a head (or the end of the array)
      const uint64_t mhx = mh | ~vm;
      uint32_t nb = __shfl_down((uint32_t)(mhx & 1ull), 1, 64);
      if (lane == 63) nb = nx_s;
      ms = mh & ((mhx >> 1) | ((uint64_t)nb << 63));
      m_sg[lane] = ms;
    }
    const uint32_t sv = (uint32_t)__popcll(vm & ~ms), hd = (uint32_t)__popcll(mh & ~ms);
    const uint32_t is = wave_incl_sum(sv), ih = wave_incl_sum(hd);
    uint32_t im;
    const uint32_t em = last_head_before_word(mh, lane, im);
    wp_s[lane] = is - sv; wp_head[lane] = em;
    if (SWEEP == 1 && lane == 63) store_tile_counts(tile_cnt, T, tile, is, ih, im ? (uint32_t)base + im : 0u);      // what bwt_flags counts
    if (SWEEP == 1) {                        // (and its large-group test: eight words to a run)
      const uint64_t nz = __ballot(mh != 0);
      if (run_without_head(nz, 8, base, A) && lane == 0) atomicOr(big_flag, 1u);
    }
  }
  __syncthreads();
  if (SWEEP == 1) carry = carry_s;
  const uint64_t lt = (1ull << lane) - 1ull, le = mask_le(lane);
  // BWT bytes of the suffixes this tile resolves (see the store below): all sixteen gathers are issued before the loop
  uint32_t ub[16];
#pragma unroll
  for (int it = 0; it < 16; it++) ub[it] = 0u;
  const bool emits = U != nullptr && SWEEP != 1;
  const uint32_t blk0 = (FIRST ? (uint32_t)base + (uint32_t)tid : p16[0]) / g.stride;      // the thread's sorted positions ascend with `it`: blk_step
  if (emits && !carried) {
    uint32_t blk = blk0;
#pragma unroll
    for (int it = 0; it < 16; it++) {
      const uint32_t e = (uint32_t)it * 256u + tid;
      const bool sing = e < nvalid && ((m_sg[it * 4 + w] >> lane) & 1ull);
      const uint32_t p = FIRST ? (uint32_t)(base + e) : p16[FIRST ? 0 : it];
      const uint32_t vv = pk_pos(PACKED ? (uint32_t)sk[e + 1] : v16[PACKED ? 0 : it]);
      blk = blk_step(p, g.stride, blk);
      ub[it] = sing ? (uint32_t)Tx[(size_t)blk * g.stride + (vv ? vv - 1u : blk_len(g, blk) - 1u)] : 0u;
    }
  }
  uint32_t blk = blk0;
#pragma unroll
  for (int it = 0; it < 16; it++) {
    const uint32_t e = (uint32_t)it * 256u + tid;
    if (e < nvalid) {
      const uint64_t a = base + e;
      const int wi = it * 4 + w;
      const uint64_t mh = m_nh[wi], ms = m_sg[wi];
      const uint64_t hm = mh & le;
      uint32_t head_a;                    // global index of the governing group head
      bool keeps_rank = false;            // the head also led the group of the previous round: R already holds this rank
      if (hm || wp_head[wi]) {
        const uint32_t hrel = hm ? (uint32_t)wi * 64u + 63u - (uint32_t)__builtin_clzll(hm) : wp_head[wi] - 1u;
        head_a = (uint32_t)base + hrel;
        if (!FIRST) keeps_rank = (m_oh[hrel >> 6] >> (hrel & 63u)) & 1ull;
      } else {
        head_a = carry - 1u;
        if (!FIRST) keeps_rank = (hflag[head_a] & HF_OLD) != 0;
      }
      const uint32_t p = FIRST ? (uint32_t)a : p16[FIRST ? 0 : it];
      const uint32_t vraw = PACKED ? (uint32_t)sk[e + 1] : v16[PACKED ? 0 : it];
      const uint32_t vv = pk_pos(vraw);                          // the suffix (positions are below 2^20)
      const uint32_t pb = PACKED ? pk2_prev(vraw) : val_prev(vraw);      // its carried byte, if any
      blk = blk_step(p, g.stride, blk);
      const uint32_t head_pos = p - ((uint32_t)a - head_a);
      if (!keeps_rank && (SWEEP == 0 || (uint32_t)(vv >= hsplit) == half)) R[(size_t)blk * g.stride + vv] = head_pos - blk * g.stride;
      if (SWEEP == 1) continue;
      if ((ms >> lane) & 1ull) {
        // a resolved suffix: its BWT byte goes straight to the output row (cyclic form: U[p] = T[suffix - 1], p in sorted-position
        // order) -- no suffix array is written, and the byte gathers overlap the rest of the regrouping instead of making a pass
        // of their own at the end; the sentinel form shifts the rows by the primary index, which is only known at the end: SA
        if (U) U[p] = (uint8_t)(carried ? pb : ub[it]);
        else __builtin_nontemporal_store(vv, SA + p);
      } else {
        const uint32_t so = sbase + wp_s[wi] + (uint32_t)__popcll(~ms & lt);
        __builtin_nontemporal_store(carried ? val_carrying(vv, pb) : vv, nval + so); __builtin_nontemporal_store(p, npos + so);
        nhead[so] = (uint8_t)((mh >> lane) & 1ull);      // a surviving head starts a group among the survivors (its group survives whole)
      }
    }
  }
}

template <typename G>
__global__ __launch_bounds__(256) void bwt_flush_active(uint32_t A, const uint32_t* __restrict__ val, const uint32_t* __restrict__ pos,
                                                        uint32_t* __restrict__ SA, G g, const uint8_t* __restrict__ Tx, uint8_t* __restrict__ U, int carried) {
  for (uint64_t a = (uint64_t)blockIdx.x * 256 + threadIdx.x; a < A; a += (uint64_t)gridDim.x * 256) {
    const uint32_t p = pos[a], v = pk_pos(val[a]);
    if (U && carried) U[p] = (uint8_t)val_prev(val[a]);
    else if (U) { const uint32_t blk = p / g.stride; U[p] = Tx[(size_t)blk * g.stride + (v ? v - 1u : blk_len(g, blk) - 1u)]; }
    else SA[p] = v;
  }
}

// primary index.  cyclic: last row of the group of rotation 0 (equal rotations are ordered by
// descending start, J/Bzip2_joined_.js:957-968); sentinel: (row of suffix 0)+1
template <typename G>
__global__ __launch_bounds__(256) void bwt_pidx(G g, int cyclic, int leftover, const uint32_t* __restrict__ R, uint32_t* __restrict__ pidx) {
  __shared__ uint32_t sm[4];
  const uint32_t blk = blockIdx.x, n = blk_len(g, blk);
  const uint32_t* r = R + (size_t)blk * g.stride;
  const uint32_t r0 = r[0];
  if (!cyclic) { if (threadIdx.x == 0) pidx[blk] = r0 + 1u; return; }
  if (!leftover) { if (threadIdx.x == 0) pidx[blk] = r0; return; }     // every rotation is unique
  uint32_t cnt = 0;
  for (uint32_t i = threadIdx.x; i < n; i += 256) cnt += r[i] == r0;
  cnt = block_sum<256>(cnt, sm);
  if (threadIdx.x == 0) pidx[blk] = r0 + cnt - 1u;
}

// BWT bytes of the sentinel form (BWTC) from the finished suffix array: rows shift by the primary index, which is only known at
// the end, so this form keeps a suffix array and an emit pass (the cyclic form writes its bytes from the regroup kernels).
// Tiles of 4096 positions, dealt to the XCDs in contiguous ranges: a block's text (the random-access side) is then
// fetched into one L2 instead of all eight; the suffix array streams through non-temporally.
__global__ __launch_bounds__(256) void bwt_emit_sentinel(const uint8_t* __restrict__ T, Geom g, uint32_t M,
                                                         const uint32_t* __restrict__ SA, const uint32_t* __restrict__ R, uint8_t* __restrict__ U, uint32_t Tn) {
  const uint32_t tile = xcd_tile(blockIdx.x, Tn);
  if (tile >= Tn) return;
#pragma unroll 4
  for (int it = 0; it < 16; it++) {
    const uint64_t a = (uint64_t)tile * RS_TILE + (uint32_t)it * 256 + threadIdx.x;
    if (a >= M) break;
    const uint32_t blk = (uint32_t)(a / g.stride), p = (uint32_t)(a - (uint64_t)blk * g.stride), n = blk_len(g, blk);
    const uint8_t* t = T + (size_t)blk * g.stride;
    uint8_t* u = U + (size_t)blk * g.stride;
    const uint32_t s = __builtin_nontemporal_load(SA + a);
    const uint32_t p0 = R[(size_t)blk * g.stride];
    if (p == p0) u[0] = t[n - 1];
    else u[p < p0 ? p + 1 : p] = t[s - 1];
  }
}

// ---- launches (bwt_parts.h).  The one place that spells out bwt_apply's arguments: the five launches of regroup differ in the template flags only.
template <bool FIRST, bool PACKED, int SWEEP, typename G>
static void launch_apply(hipStream_t s, BwtWork& w, const G& g, const Plan& p, const Round& r, uint32_t T) {
  hipLaunchKernelGGL((bwt_apply<FIRST, PACKED, SWEEP, G>), dim3(xcd_grid(T)), dim3(256), 0, s, FIRST ? w.key[r.c] : nullptr, FIRST ? nullptr : w.hflag,
                     w.val[r.c], w.pos[r.pc], r.A, g, w.tile_cnt, T, w.R, w.SA, w.val[1 - r.c], w.pos[1 - r.pc], w.ghead, HalfMap{SWEEP ? 2u : 1u, g.stride},
                     p.Tx, p.U, w.counters + CN_LARGE_GROUP, p.gs1, p.carried);
}
template <typename G>
int regroup(hipStream_t s, BwtWork& w, const G& g, const Plan& p, const Round& r) {
  const uint32_t T = (r.A + RS_TILE - 1) / RS_TILE;
  const bool first = r.rounds == 0, sweeps = first && p.sweeps;
  if (sweeps) launch_apply<true, true, 1>(s, w, g, p, r, T);            // sweep 1 counts as it goes: no counting pass (see bwt_apply)
  else if (first) hipLaunchKernelGGL(bwt_flags, dim3(T), dim3(256), 0, s, w.key[r.c], r.A, w.tile_cnt, T, p.gs1, w.counters + CN_LARGE_GROUP, g.stride);
  else hipLaunchKernelGGL(bwt_flags_bytes, dim3(T), dim3(256), 0, s, w.hflag, r.A, w.tile_cnt, T, w.counters + CN_LARGE_GROUP);
  hipLaunchKernelGGL(bwt_scan_tiles, dim3(1), dim3(1024), 0, s, w.tile_cnt, T, w.counters, w.h_counters);
  CJS_HIP_TRY(hipEventRecord(w.ev_scan, s));
  if (sweeps) launch_apply<true, true, 2>(s, w, g, p, r, T);
  else if (first && p.packed) launch_apply<true, true, 0>(s, w, g, p, r, T);
  else if (first) launch_apply<true, false, 0>(s, w, g, p, r, T);
  else launch_apply<false, false, 0>(s, w, g, p, r, T);
  return 0;
}
template int regroup<Geom>(hipStream_t, BwtWork&, const Geom&, const Plan&, const Round&);
template int regroup<VarGeom>(hipStream_t, BwtWork&, const VarGeom&, const Plan&, const Round&);

template <typename G>
void launch_gather_keys(hipStream_t s, const TsGatherT<G>& tg, uint32_t A, const uint32_t* val, uint64_t* key, uint32_t* tile_cnt) {
  const uint32_t T = (A + RS_TILE - 1) / RS_TILE;
  uint32_t* tsum = T > 2 ? tile_cnt : nullptr;      // up to two tiles (every round below tile_sorted_round): the workgroups count for themselves
  if (tsum) {
    hipLaunchKernelGGL(bwt_head_counts, dim3(T), dim3(256), 0, s, tg.ghead, A, tsum);
    hipLaunchKernelGGL(bwt_head_scan, dim3(1), dim3(1024), 0, s, tsum, T);
  }
  hipLaunchKernelGGL(bwt_gather_keys<G>, dim3(xcd_grid(T)), dim3(256), 0, s, tg.g, tg.cyclic, A, tg.h, tg.R, val, tg.pos, tg.ghead, tsum, key, T);
}
template void launch_gather_keys<Geom>(hipStream_t, const TsGatherT<Geom>&, uint32_t, const uint32_t*, uint64_t*, uint32_t*);
template void launch_gather_keys<VarGeom>(hipStream_t, const TsGatherT<VarGeom>&, uint32_t, const uint32_t*, uint64_t*, uint32_t*);
void launch_key_flags(hipStream_t s, const uint64_t* key, uint32_t A, uint8_t* hflag) {
  hipLaunchKernelGGL(bwt_key_flags, dim3((A + 255) / 256 < 8192u ? (A + 255) / 256 : 8192u), dim3(256), 0, s, key, A, hflag);
}
template <typename G>
void launch_flush_active(hipStream_t s, const BwtWork& w, const G& g, const Plan& p, const Round& r) {
  hipLaunchKernelGGL(bwt_flush_active<G>, dim3((r.A + 255) / 256), dim3(256), 0, s, r.A, w.val[r.c], w.pos[r.pc], w.SA, g, p.Tx, p.U, p.carried);
}
template void launch_flush_active<Geom>(hipStream_t, const BwtWork&, const Geom&, const Plan&, const Round&);
template void launch_flush_active<VarGeom>(hipStream_t, const BwtWork&, const VarGeom&, const Plan&, const Round&);
template <typename G>
void launch_finish(hipStream_t s, const BwtWork& w, const G& g, bool cyclic, bool leftover, uint32_t M, const uint8_t* d_T, uint8_t* d_U, uint32_t* d_pidx) {
  hipLaunchKernelGGL(bwt_pidx<G>, dim3(g.nb), dim3(256), 0, s, g, (int)cyclic, (int)leftover, w.R, d_pidx);
  if constexpr (std::is_same_v<G, Geom>) if (!cyclic) {
    const uint32_t Tn = (M + RS_TILE - 1) / RS_TILE;
    hipLaunchKernelGGL(bwt_emit_sentinel, dim3(xcd_grid(Tn)), dim3(256), 0, s, d_T, g, M, w.SA, w.R, d_U, Tn);
  }
}
template void launch_finish<Geom>(hipStream_t, const BwtWork&, const Geom&, bool, bool, uint32_t, const uint8_t*, uint8_t*, uint32_t*);
template void launch_finish<VarGeom>(hipStream_t, const BwtWork&, const VarGeom&, bool, bool, uint32_t, const uint8_t*, uint8_t*, uint32_t*);

}  // namespace cjs
