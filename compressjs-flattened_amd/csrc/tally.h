// tally.h -- what the key tally (tally.hip) offers the stream consumer that feeds it keys in device memory
// (cjs_bzip2_tally, tally_stream.hip): its workspace, sized from the number of keys alone, and the run into a host array.
#pragma once
#include "cjs_internal.h"
#include "tally_plan.h"

namespace cjs {

constexpr uint32_t TL_TILE = 1024;      // slots (or groups) of a workgroup: 256 threads x 4, slot = tile * 1024 + round * 256 + thread
enum TlScalar { TL_N_BAD = 0, TL_N_DISTINCT = 1, TL_N_GROUPS = 2, TL_MAX_COUNT = 3, TL_SCALARS = 4 };

// What a tally of n keys holds on the device beyond the keys and the groups written: 37 bytes a key (two 8-byte and two 4-byte
// sort buffers, a flag byte, first / count / order value of the kept groups), two counts per tile, the sorter's histograms.
struct TallyWork {
  uint64_t* k[2] = {nullptr, nullptr};
  uint32_t* v[2] = {nullptr, nullptr};
  uint8_t* flag = nullptr;
  uint32_t *cfirst = nullptr, *ccount = nullptr, *ov = nullptr;
  uint64_t *tcnt = nullptr, *taux = nullptr, *scal = nullptr;
  RadixWork rs;
  static size_t tiles(size_t n) { return (n + TL_TILE - 1) / TL_TILE; }
  static size_t bytes_needed(size_t n) {
    auto pad = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t ht = RadixWork::hist_tiles_for(n);
    return 2 * pad(8 * n) + 5 * pad(4 * n) + pad(n) + 2 * pad(8 * tiles(n)) + pad(8 * TL_SCALARS) + pad(4 * RadixWork::hist_words(ht)) + pad(4 * 256);
  }
  int carve(Arena& a, size_t n) {
    for (int i = 0; i < 2; i++) { k[i] = a.take<uint64_t>(n); v[i] = a.take<uint32_t>(n); }
    flag = a.take<uint8_t>(n);
    cfirst = a.take<uint32_t>(n); ccount = a.take<uint32_t>(n); ov = a.take<uint32_t>(n);
    tcnt = a.take<uint64_t>(tiles(n)); taux = a.take<uint64_t>(tiles(n)); scal = a.take<uint64_t>(TL_SCALARS);
    if (!k[0] || !k[1] || !v[0] || !v[1] || !flag || !cfirst || !ccount || !ov || !tcnt || !taux || !scal) return CJS_E_OUT_OF_MEMORY;
    return rs.carve(a, RadixWork::hist_tiles_for(n), 1);
  }
};

// d_keys[0 .. n), 0 < n <= TL_MAX_KEYS, grouped on stream s in workspace w (carved for n keys or more): info, and the first
// min(cap, n_groups) groups into the HOST array out, their `first` raised by first_base.  They pass through d_stage, device memory
// for min(cap, n) records (nullptr: taken from the pool once n_groups is known).  Returns with s drained.
int tally_to_host(hipStream_t s, TallyWork& w, const cjs_bz_linekey* d_keys, uint32_t n, uint32_t order, uint64_t min_count, uint64_t max_count,
                  uint64_t first_base, cjs_bz_tally* out, size_t cap, cjs_tally_info* info, cjs_bz_tally* d_stage = nullptr);

}  // namespace cjs
