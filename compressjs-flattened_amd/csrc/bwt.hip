// bwt.hip — batched suffix sorting / Burrows-Wheeler transform for gfx950: the workspace, the plan of round 1 and the round loop.
// Host code only.  The kernels, by role, each file behind the plain functions of bwt_parts.h that queue its launches:
//   bwt_round1.hip     sort_round1: keys of the unsegmented round 1, record rebuild of the packed two-phase round 1
//   bwt_tile_sort.hip  the two tile sorters of the rounds >= 2 and their shared window prologue
//   bwt_defer.hip      the trip of the groups too large for the tile sorters: count, scan | gather, sort, scatter back
//   bwt_regroup.hip    regroup behind every sort, the keys / flag bytes of the whole-array fallbacks, the emit passes
//   bwt_dev.hpp        device helpers that several of them share;  bwt_rules.h  the rules they must agree on, no HIP
//
// Replaces BWT.bwtransform2 (cyclic; J/Bzip2_joined_.js:928-971 -> SA_IS :730-857) and
// BWT.bwtransform (sentinel; J/BWTC_joined_.js:1125-1145) for ALL blocks of a batch at once.
// The reference runs SA-IS (serial induced sorting) per block.  A suffix array is unique, so
// any correct construction gives the same BWT; here it is prefix doubling (Manber-Myers /
// Larsson-Sadakane) expressed as data-parallel passes over all blocks' suffixes together.
//
// Round 1 sorts every suffix by its leading 7 symbols (fewer when the block id has to share the key) with the segmented radix
// sorter of radix.hip, one segment per block:
//   cyclic    packed two-phase records and no value array: bytes 2..6 first (one u64 per suffix for two passes, one u32 = byte 2 |
//             position for the last three), then bwt_phase2_records rebuilds the records as bytes 0..1 | rank of the class of
//             bytes 2..6 | the byte in front | position, and two more passes finish depth 7
//   sentinel  (u64 key, u32 value) records, 9-bit symbols
//   fallback  more blocks or tiles than the workspace has segments for, several blocks shorter than a 4096-slot tile, blocks of
//             different lengths (bwt_run_var), or CJS_NO_SEGMENTED_SORT: bwt_init_keys writes keys with the block id on top,
//             sorted as one array
// Rounds >= 2 sort only the suffixes of unresolved groups, by (group ordinal, rank of suffix + h), h = 7, 14, 28, ...  The array
// is already ordered by group, so the tile sorters order every group of <= 1024 suffixes in LDS and fetch the ranks themselves;
// larger groups are deferred: compacted, radix-sorted apart, scattered back.  Whole-array fallbacks (radix passes over keys that
// bwt_gather_keys writes): fewer than 8192 unresolved suffixes, or more than half of the workspace deferred.
// Every round ends in a regroup: new ranks into R, resolved suffixes out (cyclic: their BWT byte straight into the output;
// sentinel: into SA), survivors compacted, each with one head byte (ghead[]: 1 = starts a group of the new grouping).  That byte is
// all the next sort is told about the groups: the tile sorters lay the bytes over their mask words, the deferral kernels number the
// groups they get from the head bit that the sorters leave in the keys, and bwt_gather_keys counts group ordinals out of the bytes.
// The host reads the survivor and group counts behind the tile scan and queues the next round.  Cyclic blocks with h >= the block
// length hold only equal rotations: bwt_flush_active emits them as they stand.
//
// Launches of one round, in order ([..]: only when the condition holds):
//   sort, round 1    [fallback: bwt_init_keys]  radix passes (rs_hist | rs_hist_bytes, rs_scan_*, rs_scatter per digit)
//                    [packed: bwt_phase2_records, two more radix passes]
//   sort, round >= 2 [large groups possible: dev_fill dflag]  bwt_tile_sort | bwt_tile_sort_radix
//                    [large groups possible: bwt_defer_count, scan_u32_single x 2, HOST WAIT; if any:
//                     bwt_defer_gather, radix passes, bwt_defer_scatter | over half deferred: bwt_gather_keys, whole-array sort]
//     whole array:   radix passes, bwt_key_flags   (keys: [more than two tiles: bwt_head_counts, bwt_head_scan] bwt_gather_keys)
//   regroup          bwt_flags (round 1) | bwt_flags_bytes -> bwt_scan_tiles -> event -> bwt_apply
//                    round 1, packed, >= 8 blocks: bwt_apply sweep 1 -> bwt_scan_tiles -> event -> bwt_apply sweep 2
//   HOST WAIT on the event; then [equal rotations only: bwt_flush_active, done]  [next round whole-array: bwt_gather_keys]
// After the last round: bwt_pidx, [sentinel: bwt_emit_sentinel].
//
// Integer sort/scan only (no MFMA); HBM-bound on the radix scatter passes.
#include "bwt_parts.h"
#include <stdlib.h>
#include <type_traits>

namespace cjs {

size_t BwtWork::bytes_needed(size_t cap) {
  const size_t T = RadixWork::hist_tiles_for(cap);
  size_t b = 0;
  auto add = [&](size_t n) { b += (n + 255) & ~(size_t)255; };
  add(cap * 8); add(cap * 8); add(cap * 4); add(cap * 4); add(cap * 4); add(cap * 4);  // key x2, val x2, pos x2
  add(cap * 4); add(cap * 4); add(cap); add(cap); add(cap);  // R, SA, dflag, hflag, ghead
  add(RadixWork::hist_words(T) * 4); add(256 * RadixWork::segs_for(cap) * 4); add(3 * T * 4); add(64);
  return b + 4096;
}
int BwtWork::carve(Arena& a, size_t cap_) {
  cap = cap_;
  const size_t T = RadixWork::hist_tiles_for(cap);
  key[0] = a.take<uint64_t>(cap); key[1] = a.take<uint64_t>(cap);
  val[0] = a.take<uint32_t>(cap); val[1] = a.take<uint32_t>(cap);
  pos[0] = a.take<uint32_t>(cap); pos[1] = a.take<uint32_t>(cap);
  R = a.take<uint32_t>(cap); SA = a.take<uint32_t>(cap); dflag = a.take<uint8_t>(cap); hflag = a.take<uint8_t>(cap); ghead = a.take<uint8_t>(cap);
  CJS_TRY(rs.carve(a, T, RadixWork::segs_for(cap)));
  tile_cnt = a.take<uint32_t>(3 * T); counters = a.take<uint32_t>(16);
  if (!counters) return CJS_E_OUT_OF_MEMORY;
  if (!h_counters) CJS_HIP_TRY(hipHostMalloc((void**)h_counters.put(), 64));
  if (!ev_scan) CJS_HIP_TRY(hipEventCreateWithFlags(ev_scan.put(), hipEventDisableTiming));
  return 0;
}

template <typename G>
static Plan plan_round1(const BwtWork& w, const G& g, bool cyclic, const uint8_t* d_T, uint8_t* d_U) {
  constexpr bool VAR = std::is_same_v<G, VarGeom>;
  Plan p;
  const uint32_t tps = ((g.nb > 1 ? g.stride : g.n_last) + RS_TILE - 1) / RS_TILE;
  // Segmented keys carry no block id, and the regroup of round 1 (bwt_flags, bwt_apply) takes ONE block start per 4096-slot tile
  // as a head: blocks shorter than a tile, several to a tile, keep the block id in the key (equal blocks would merge otherwise)
  const bool blocks_share_tiles = g.nb > 1 && g.stride < RS_TILE;
  p.segmented = !VAR && !blocks_share_tiles && (uint64_t)g.nb * tps <= w.rs.hist_tiles && g.nb <= w.rs.bintot_segs &&
                getenv("CJS_NO_SEGMENTED_SORT") == nullptr;
  p.packed = p.segmented && cyclic;
  p.sweeps = g.nb >= 8 && p.packed;
  const Round1Keys k = round1_keys(g.nb, cyclic, p.segmented, VAR);
  p.nsym = k.nsym; p.bits = k.bits;
  p.gs1 = p.packed ? PK2_GSHIFT : 0;
  p.carried = p.packed ? 1 : 0;
  p.sg = SegGeom{g.nb, g.stride, g.n_last, tps};
  p.gen = GenSrc{d_T, cyclic ? 1 : 0, p.nsym, p.packed ? 2 : 0};
  p.Tx = cyclic ? d_T : nullptr; p.U = cyclic ? d_U : nullptr;
  return p;
}

// whole-array fallback of a round >= 2: radix passes over the 64-bit keys in key[c], then the flag bytes from the sorted keys
static int sort_round_whole(hipStream_t s, BwtWork& w, Round& r, LaunchTimes* lt) {
  // (whole digits are sorted: the rest of the last one is zero, bwt_gather_keys' round_key(ord, rank) has ord < ngroups on top)
  CJS_TRY((radix_passes<uint64_t>(s, w.rs, w.key[0], w.val[0], w.key[1], w.val[1], r.c, r.A, 0, r.bits, lt)));
  launch_key_flags(s, w.key[r.c], r.A, w.hflag);
  CJS_HIP_TRY(hipGetLastError());
  return 0;
}
// One sort of a round >= 2: in-LDS tile sort of the small groups + global radix passes for the large ones.
// Works in place on val[c] and leaves the head flags of the sorted order in hflag[]; only the whole-array fallback flips c.
// key[c] only ever holds the keys of the slots the tile sorters do not own (the deferral kernels read them).
template <typename TG>
static int sort_round(hipStream_t s, BwtWork& w, Round& r, LaunchTimes* lt, const TG& tg) {
  if (!tile_sorted_round(r.A)) return sort_round_whole(s, w, r, lt);      // (bwt_gather_keys made the keys)
  const uint32_t A = r.A;
  const int c = r.c;
  uint32_t* tcount = w.tile_cnt;                        // 3*cap/4096 entries >= cap/2048
  if (r.no_large_groups) {                              // groups only ever split: once none exceeds TS_MAXGRP, none will
    launch_tile_sort(s, w.key[c], w.val[c], w.hflag, A, nullptr, r.ngroups, tg);
    CJS_HIP_TRY(hipGetLastError());
    return 0;
  }
  dev_fill(s, w.dflag, 1, A);
  launch_tile_sort(s, w.key[c], w.val[c], w.hflag, A, w.dflag, r.ngroups, tg);
  uint32_t* hcount = w.rs.hist;                         // (free between sorts: the radix passes below come after the last reader of hcount)
  launch_defer_count(s, A, w.dflag, w.key[c], tcount, hcount, w.counters, w.h_counters);
  CJS_HIP_TRY(hipStreamSynchronize(s));
  const uint32_t D = w.h_counters[CN_DEFERRED];
  if (env_debug()) fprintf(stderr, "[cjs bwt]   tile sort: %u of %u suffixes in groups > %u\n", D, A, TS_MAXGRP);
  if (D == 0) { r.no_large_groups = true; return 0; }
  if (deferred_overflow(D, w.cap)) {       // no room to sort them apart: the whole array by its keys (the sorted slots hold none: gathered again)
    launch_gather_keys(s, tg, A, w.val[c], w.key[c], w.tile_cnt);      // (tcount is dead behind the host wait)
    return sort_round_whole(s, w, r, lt);
  }
  CJS_TRY(sort_deferred(s, w, r, D, w.h_counters[CN_DEFERRED_GROUPS], tcount, hcount, lt));
  CJS_HIP_TRY(hipGetLastError());
  return 0;
}

// Behind a regroup: the keys of the next sort, its depth and its key bits
template <typename G>
static void prepare_next(hipStream_t s, BwtWork& w, const G& g, bool cyclic, Round& r, TsGatherT<G>& tg) {
  tg = TsGatherT<G>{w.R, w.pos[r.pc], w.ghead, r.h, (int)cyclic, g};
  if (!tile_sorted_round(r.A)) launch_gather_keys(s, tg, r.A, w.val[r.c], w.key[r.c], w.tile_cnt);      // (else the tile sorters fetch the ranks themselves)
  r.h = next_depth(r.h);
  r.bits = round_key_bits(r.ngroups);
}

// G = Geom: every block `stride` long but the last (n_last).  G = VarGeom: block k is g.len[k] <= stride long, every slot of
// the array is `stride` wide (n_last == stride), and round 1 takes the unsegmented path with the hole bit (bwt_init_keys).
template <typename G>
static int bwt_run_impl(hipStream_t s, BwtWork& w, const uint8_t* d_T, const G g, bool cyclic, uint8_t* d_U, uint32_t* d_pidx,
                        cjs_stats* stats, bool resolve_stats) {
  constexpr bool VAR = std::is_same_v<G, VarGeom>;
  const uint32_t nb = g.nb, stride = g.stride, n_last = g.n_last;
  if (nb == 0) return 0;
  if (VAR && (!cyclic || n_last != stride)) return CJS_E_INVALID_ARG;
  const uint64_t M64 = (uint64_t)(nb - 1) * stride + n_last;
  if (M64 > w.cap || !bwt_admits(M64, stride)) return CJS_E_INVALID_ARG;      // slots are 32 bits wide, ranks must fit 20 bits
  const uint32_t M = (uint32_t)M64;
  const uint32_t max_n = nb > 1 ? stride : n_last;
  LaunchTimes& lt = w.lt; lt.reset(); lt.enabled = stats != nullptr; lt.min_elems = M;      // the roofline is priced on the full-size scatter passes
  const Plan p = plan_round1(w, g, cyclic, d_T, d_U);
  if (VAR && !var_geom_admits(p.nsym)) return CJS_E_INVALID_ARG;                 // a hole's position must fit its symbol bits

  dev_fill(s, w.counters, 0, 64);
  Round r;
  r.A = M; r.h = (uint32_t)p.nsym; r.bits = p.bits;
  TsGatherT<G> tg{nullptr, nullptr, nullptr, 0u, 0, g};
  for (;;) {
    if (r.rounds == 0) CJS_TRY(sort_round1(s, w, g, p, r, &lt));
    else CJS_TRY(sort_round(s, w, r, &lt, tg));
    CJS_TRY(regroup(s, w, g, p, r));
    // the host only needs the counters of the tile scan: it waits for THAT kernel and queues the next round behind the regroup
    // kernel while it runs (a stream synchronisation here left the GPU idle for ~20 us per round)
    CJS_HIP_TRY(hipEventSynchronize(w.ev_scan));
    r.rounds++;
    const uint32_t A2 = w.h_counters[CN_SURVIVORS], NG = w.h_counters[CN_GROUPS];
    if (w.h_counters[CN_LARGE_GROUP] == 0) r.no_large_groups = true;       // every group of the new grouping fits the tile sorters
    if (env_debug()) fprintf(stderr, "[cjs bwt] round %u h=%u A=%u bits=%d -> A'=%u groups=%u\n", r.rounds, r.h, r.A, r.bits, A2, NG);
    r.c = 1 - r.c; r.pc = 1 - r.pc;
    r.A = A2; r.ngroups = NG;
    if (r.A == 0) break;
    if (cyclic && r.h >= max_n) {     // only groups of equal rotations are left
      launch_flush_active(s, w, g, p, r);
      break;
    }
    if (r.rounds > 40) return CJS_E_HIP;    // cannot happen: depth doubles every round
    prepare_next(s, w, g, cyclic, r, tg);
  }
  launch_finish(s, w, g, cyclic, r.A != 0, M, d_T, d_U, d_pidx);
  CJS_HIP_TRY(hipGetLastError());
  if (stats) stats->bwt_rounds = r.rounds;
  if (stats && resolve_stats) {                  // (else the caller resolves w.lt once its stream has drained)
    CJS_HIP_TRY(hipStreamSynchronize(s));
    lt.resolve(stats);
  }
  return 0;
}

int bwt_run(hipStream_t s, BwtWork& w, const uint8_t* d_T, uint32_t nb, uint32_t stride, uint32_t n_last,
            bool cyclic, uint8_t* d_U, uint32_t* d_pidx, cjs_stats* stats, bool resolve_stats) {
  return bwt_run_impl(s, w, d_T, Geom{nb, stride, n_last}, cyclic, d_U, d_pidx, stats, resolve_stats);
}

int bwt_run_var(hipStream_t s, BwtWork& w, const uint8_t* d_T, uint32_t nb, uint32_t stride, const uint32_t* d_len,
                uint8_t* d_U, uint32_t* d_pidx) {
  return bwt_run_impl(s, w, d_T, VarGeom{nb, stride, stride, d_len}, true, d_U, d_pidx, nullptr, true);
}

}  // namespace cjs
