// bwt_round1.hip — round 1 of the suffix sort (the map: bwt.hip): the keys of its unsegmented form, and the record rebuild between
// the two phases of the packed form, which reads the 4-byte records that phase 1 ends on and takes every slot's class key back
// from the block text.  The radix passes themselves are radix.hip; the key and record layouts are bwt_rules.h.
#include "bwt_dev.hpp"

namespace cjs {

// keys of the unsegmented round 1: (block id, first nsym symbols).  cyclic: bytes wrap; sentinel: 9-bit symbols, 0 = past the end
// VarGeom: one more bit between the block id and the symbols flags a hole; a hole's symbols are its position (unique)
template <typename G>
__global__ __launch_bounds__(256) void bwt_init_keys(const uint8_t* __restrict__ T, G g, int cyclic, int nsym, uint32_t M,
                                                     uint64_t* __restrict__ key, uint32_t* __restrict__ val) {
  for (uint64_t a = (uint64_t)blockIdx.x * 256 + threadIdx.x; a < M; a += (uint64_t)gridDim.x * 256) {
    const uint32_t blk = (uint32_t)(a / g.stride), i = (uint32_t)(a - (uint64_t)blk * g.stride), n = blk_len(g, blk);
    const uint8_t* t = T + (size_t)blk * g.stride;
    uint64_t k = 0;
    if constexpr (std::is_same_v<G, VarGeom>) {
      uint32_t x = i;
      if (i >= n) k = (1ull << r1_hole_bit(nsym)) | i;
      else for (int j = 0; j < nsym; j++) { k = (k << 8) | t[x]; if (++x == n) x = 0; }
      k |= (uint64_t)blk << (r1_hole_bit(nsym) + 1);
    } else if (cyclic) {
      uint32_t x = i;
      for (int j = 0; j < nsym; j++) { k = (k << 8) | t[x]; if (++x == n) x = 0; }
      k |= (uint64_t)blk << r1_block_shift(true, nsym);
    } else {
      for (int j = 0; j < nsym; j++) { const uint32_t x = i + j; k = (k << 9) | (x < n ? (uint32_t)t[x] + 1u : 0u); }
      k |= (uint64_t)blk << r1_block_shift(false, nsym);
    }
    key[a] = k; val[a] = i;                // slot a of round 1 is sorted position a: no pos[] yet
  }
}

// Two-phase round 1 (cyclic, packed records): seven bytes of depth.  Phase 1 sorted every block by bytes 2..6 and ends on the
// narrow records of its last passes (byte 2 | position, 4 bytes: bwt_rules.h); here every sorted slot learns r1 = block-local slot
// of the head of its (bytes 2..6) class and becomes the phase-2 record  byte0 . byte1 (bits 63..48) | r1 (47..28) | the byte in
// front (27..20) | position (19..0); two more stable passes on the top 16 bits then order by (byte0, byte1, class of bytes 2..6),
// and key >> 28 is the 7-byte group key.
// The class key of a slot is no longer in its record: it comes back from the block text, with the bytes in front and at the
// suffix that this kernel gathers anyway -- text[p - 1 .. p + 6] as three aligned words (text8 of bwt_dev.hpp), which lie in one
// 64-byte line about nine times out of ten.  So do the keys of the slot in front of the tile and of the class search's probes.
// Tiles are the tiles of the segmented radix passes (one segment per block), so this kernel also leaves the per-tile
// histogram of byte1 -- the digit of the first phase-2 pass -- in hist[], and that pass needs no rs_hist of its own.
// No flag / scan passes in front either: the only class head a tile cannot see is the one of the class that runs into it,
// and the block is sorted, so wave 0 finds it by looking at the 64 slots in front of the tile (nearly always enough) and
// otherwise by a 64-way search for the lower bound of the tile's first key in the block.
__global__ __launch_bounds__(256) void bwt_phase2_records(const uint32_t* __restrict__ rec, SegGeom sg, const uint8_t* __restrict__ T,
                                                          uint32_t* __restrict__ hist, uint64_t* __restrict__ out) {
  __shared__ uint64_t sk[RS_TILE + 1];
  __shared__ uint64_t m_nh[64];
  __shared__ uint32_t wp_head[64];
  constexpr int PH = 2;                          // histogram copies per wave (the 32 KB of sk[] limit the residency already)
  __shared__ uint32_t h[4 * 256 * PH];
  __shared__ uint32_t carry_s;
  const uint32_t tile = blockIdx.x;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const TileRef t = tile_ref(sg, tile);
  if (!t.nvalid) { hist[(size_t)tile * 256 + tid] = 0; return; }
  const uint64_t base = t.base, seg0 = (uint64_t)t.seg * sg.stride;
  const uint32_t nvalid = t.nvalid, n = t.seg + 1 == sg.nseg ? sg.n_last : sg.stride;
  const uint8_t* tx = T + seg0;
  uint32_t p16[16];                              // all loads first (see bwt_apply)
#pragma unroll
  for (int it = 0; it < 16; it++) {
    const uint32_t e = (uint32_t)it * 256u + tid;
    p16[it] = pk_pos(__builtin_nontemporal_load(rec + base + (e < nvalid ? e : nvalid - 1u)));
  }
  const auto class_at = [&](uint64_t i) { return pk_key_of_text(text8(tx, pk_pos(rec[i]), n)); };
  if (tid == 64) sk[0] = t.off ? class_at(base - 1) : ~0ull;
  if (w == 0) {
    // head of the class of the tile's first slot (global index + 1, as bwt_scan_tiles would have carried it)
    const uint32_t carry = (uint32_t)class_head_before_by(class_at, seg0, base, lane) + 1u;
    if (lane == 0) carry_s = carry;
  }
  // the eight text bytes around every record's suffix: gathers from the block text (L2), all issued before the first is used
  uint64_t t16[16];
#pragma unroll
  for (int it = 0; it < 16; it++) t16[it] = text8_words(tx, p16[it], n);
#pragma unroll
  for (int it = 0; it < 16; it++)
    if (text8_wraps(p16[it], n)) t16[it] = text8_wrapping(tx, p16[it], n);      // (seven positions of a block)
  uint32_t b01[16];                              // byte 0 . byte 1 | the byte in front << 16: carried from here on
#pragma unroll
  for (int it = 0; it < 16; it++) b01[it] = pk_bytes01_of_text(t16[it]) | (pk_prev_of_text(t16[it]) << 16);
#pragma unroll
  for (int i = 0; i < 4 * PH; i++) h[i * 256 + tid] = 0;
#pragma unroll
  for (int it = 0; it < 16; it++) {
    const uint32_t e = (uint32_t)it * 256u + tid;
    sk[e + 1] = e < nvalid ? pk_key_of_text(t16[it]) : ~0ull;
  }
  __syncthreads();
  uint32_t* hw = h + w * 256 * PH + (tid & (PH - 1));      // (bank-interleaved copies as in rs_hist)
#pragma unroll
  for (int it = 0; it < 16; it++) {
    const uint32_t e = (uint32_t)it * 256u + tid;
    const bool nh = e < nvalid && (t.off + e == 0 || sk[e] != sk[e + 1]);
    const uint64_t mnh = __ballot(nh);
    if (lane == 0) m_nh[it * 4 + w] = mnh;
    if (e < nvalid) atomicAdd(&hw[(b01[it] & 255u) * PH], 1u);
  }
  __syncthreads();
  if (w == 0) {
    const uint64_t mh = m_nh[lane];
    uint32_t im;
    wp_head[lane] = last_head_before_word(mh, lane, im);
  }
  {
    uint32_t sum = 0;
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int r = 0; r < PH; r++) sum += h[i * 256 * PH + tid * PH + r];
    hist[(size_t)tile * 256 + tid] = sum;
  }
  __syncthreads();
  const uint32_t carry = carry_s;
  const uint64_t le = mask_le(lane);
#pragma unroll
  for (int it = 0; it < 16; it++) {
    const uint32_t e = (uint32_t)it * 256u + tid;
    if (e < nvalid) {
      const int wi = it * 4 + w;
      const uint64_t hm = m_nh[wi] & le;
      const uint32_t head_a = hm ? (uint32_t)base + (uint32_t)wi * 64u + 63u - (uint32_t)__builtin_clzll(hm) : wp_head[wi] ? (uint32_t)base + wp_head[wi] - 1u : carry - 1u;
      const uint32_t r1 = head_a - (uint32_t)seg0;
      __builtin_nontemporal_store(pk2_record(b01[it], r1, b01[it] >> 16, p16[it]), out + base + e);
    }
  }
}

// The sort of round 1 by the plan: unsegmented | segmented | segmented and packed (two phases)
template <typename G>
int sort_round1(hipStream_t s, BwtWork& w, const G& g, const Plan& p, Round& r, LaunchTimes* lt) {
  if (!p.segmented) {
    const int grid_lin = (int)((r.A + 255) / 256 < 65535u * 16u ? (r.A + 255) / 256 : 65535u * 16u);
    hipLaunchKernelGGL(bwt_init_keys<G>, dim3(grid_lin), dim3(256), 0, s, p.gen.T, g, p.gen.cyclic, p.nsym, r.A, w.key[0], w.val[0]);
    // (whole digits are sorted: the rest of the last one is zero, bwt_init_keys puts nothing above the block id, r.bits = p.bits wide)
    return radix_passes<uint64_t>(s, w.rs, w.key[0], w.val[0], w.key[1], w.val[1], r.c, r.A, 0, r.bits, lt);
  }
  // (r.bits = 63: the last digit takes in bit 63, the segment's parity in gen_key -- equal in all keys of a segment, so it moves nothing)
  if (!p.packed) return radix_passes<uint64_t>(s, w.rs, w.key[0], w.val[0], w.key[1], w.val[1], r.c, r.A, 0, r.bits, lt, &p.sg, &p.gen);
  // phase 1: its narrow records go through val[], which the packed round 1 does not use before the regroup writes the next
  // round's values (behind the rebuild that consumes them).  The 8-byte records of the first passes in key[] are dead by then:
  // the rebuild writes key[r.c]
  CJS_TRY(radix_passes_pk1(s, w.rs, w.key[0], w.key[1], w.val[0], w.val[1], r.A, lt, p.sg, p.gen, w.dflag));
  hipLaunchKernelGGL(bwt_phase2_records, dim3(p.sg.nseg * p.sg.tps), dim3(256), 0, s, w.val[0], p.sg, p.gen.T, w.rs.hist, w.key[r.c]);
  return radix_passes<uint64_t>(s, w.rs, w.key[0], w.val[0], w.key[1], w.val[1], r.c, r.A, 48, 64, lt, &p.sg, nullptr, true, true, w.dflag);
}
template int sort_round1<Geom>(hipStream_t, BwtWork&, const Geom&, const Plan&, Round&, LaunchTimes*);
template int sort_round1<VarGeom>(hipStream_t, BwtWork&, const VarGeom&, const Plan&, Round&, LaunchTimes*);

}  // namespace cjs
