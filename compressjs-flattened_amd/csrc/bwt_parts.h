// bwt_parts.h — what the round loop of the suffix sort (bwt.hip, host code only) shares with the files that hold its kernels: the
// block geometries, the plan of round 1, the state of a run, and the launch functions that bwt.hip calls across translation
// units.  Kernels templated on the geometry are instantiated in the file that defines them, behind these functions.
#pragma once
#include "radix.hpp"

namespace cjs {

struct Geom { uint32_t nb, stride, n_last; };
// Blocks of different lengths in slots of one stride (a batch of independent inputs: one block per input, bwt_run_var).
// Slot positions at or past a block's length are holes: round 1 gives them keys that sort behind the block's suffixes and
// resolve as singletons there, so no later round sees them.  The kernels take the geometry as a template parameter: the
// fixed-geometry instantiation (bwt_run) is the code it was before.
struct VarGeom { uint32_t nb, stride, n_last; const uint32_t* len; };

// Round 1, decided once per run (the forms: file header of bwt.hip).  Segmented: keys generated from the block bytes in the
// first pass, 7 symbols + the block parity.  Packed (same-box A/Bs in profiles/r02_*): the seven passes + the record rebuild
// cost more than five passes, but 61 M instead of 83.5 M suffixes stay unresolved behind them and every suffix-round costs
// ~55 ps; their scatter passes leave the next digit of every key as a byte for the next pass's counts.
struct Plan {
  bool segmented, packed;
  bool sweeps;                        // two-sweep rank scatter of round 1 (see HalfMap): pays only with the packed records (the second sweep of the 12-byte form re-reads more than the merged stores save: 2.15 vs 1.64 ms)
  int nsym, bits;                     // symbols and key bits of the round-1 sort
  int gs1, carried;                   // group key of the round-1 records = key >> gs1; the records (then val[]) carry the byte in front of their suffix
  SegGeom sg; GenSrc gen;
  const uint8_t* Tx; uint8_t* U;      // cyclic form: the regroup kernels write the BWT bytes of the suffixes they resolve themselves; sentinel form: null, it keeps a suffix array
};

// What a run carries from round to round.
struct Round {
  int c = 0, pc = 0;                 // which key / val buffer and which pos buffer hold the active arrays
  uint32_t A = 0, h = 0;             // active (unresolved) suffixes; depth they are sorted to
  int bits = 0;                      // key bits of the next sort
  uint32_t ngroups = 0, rounds = 0;  // groups among the active suffixes; rounds done
  bool no_large_groups = false;      // no unresolved group exceeds the tile sorters' limit any more
};

// Arguments of the fused rank gather of the tile sorters (bwt_tile_sort.hip)
template <typename G> struct TsGatherT { const uint32_t* R; const uint32_t* pos; const uint8_t* ghead; uint32_t h; int cyclic; G g; };

// Every function below is instantiated for G = Geom and VarGeom (TG = TsGatherT of them) and queues its launches on s.
// bwt_round1.hip: the sort of round 1 ([bwt_init_keys] radix passes [bwt_phase2_records, radix passes]); flips r.c as the passes do
template <typename G> int sort_round1(hipStream_t s, BwtWork& w, const G& g, const Plan& p, Round& r, LaunchTimes* lt);
// bwt_tile_sort.hip: one of the two tile sorters over the ts_windows(A) windows
template <typename TG> void launch_tile_sort(hipStream_t s, uint64_t* key, uint32_t* val, uint8_t* hflag, uint32_t A, uint8_t* dflag, uint32_t ngroups, const TG& tg);
// bwt_defer.hip: the trip of the groups that the tile sorters leave (dflag = 1).  Count: per TS_GT tile, then the scans of both
// counts, which write the totals to counters[CN_DEFERRED*] and to their pinned mirror themselves.  Then, for D > 0 slots in ndg
// groups: bwt_defer_gather into the spare halves of the workspace, radix passes, bwt_defer_scatter
void launch_defer_count(hipStream_t s, uint32_t A, const uint8_t* dflag, const uint64_t* key, uint32_t* tcount, uint32_t* hcount, uint32_t* counters, uint32_t* h_counters);
int sort_deferred(hipStream_t s, BwtWork& w, const Round& r, uint32_t D, uint32_t ndg, const uint32_t* tcount, const uint32_t* hcount, LaunchTimes* lt);
// bwt_regroup.hip.  regroup: per-tile counts, their scan (w.ev_scan behind it is what the host waits for), then bwt_apply
template <typename G> int regroup(hipStream_t s, BwtWork& w, const G& g, const Plan& p, const Round& r);
// (the keys' group ordinals are counted from the head bytes: tile_cnt takes the per-tile sums when A spans more than two tiles)
template <typename G> void launch_gather_keys(hipStream_t s, const TsGatherT<G>& tg, uint32_t A, const uint32_t* val, uint64_t* key, uint32_t* tile_cnt);
void launch_key_flags(hipStream_t s, const uint64_t* key, uint32_t A, uint8_t* hflag);
template <typename G> void launch_flush_active(hipStream_t s, const BwtWork& w, const G& g, const Plan& p, const Round& r);
template <typename G> void launch_finish(hipStream_t s, const BwtWork& w, const G& g, bool cyclic, bool leftover, uint32_t M, const uint8_t* d_T, uint8_t* d_U, uint32_t* d_pidx);      // bwt_pidx, [sentinel: bwt_emit_sentinel]

}  // namespace cjs
