// stage_radix.hip — cjs_stage_radix, the stage-level entry point of the radix sorter (radix.hip).  EXISTS FOR TESTS; no product path
// calls it.  Host buffers in and out, an arena and a stream of its own, like the entries of stages.hip.  The sorter's callers each
// fix their own template arguments, bit range and geometry; this entry takes them as arguments, carves the RadixWork as the
// product's workspaces carve it (hist_tiles_for / segs_for of a capacity), fills everything the passes write to with a byte first
// (the product reuses its workspaces: every pass meets stale counts) and puts guards behind the arrays.  It adds nothing to
// radix.hip but the calls of radix_passes and radix_pass_segments.
#include "cjs_internal.h"
#include "host.h"
#include "radix.hpp"
#include <vector>

using namespace cjs;

namespace {

constexpr size_t RX_GUARD = 1024;                 // bytes of guard behind each key, value and byte array
constexpr size_t RX_MAX_CAP = (size_t)1 << 26;    // keys the workspace may be carved for (bounds the arena: ~30 bytes a key)
constexpr uint32_t RX_FLAGS = CJS_RADIX_DIG | CJS_RADIX_SEGMENTS | CJS_RADIX_FIRST_HIST | CJS_RADIX_GEN;

// an array of `bytes` bytes with its guard behind it, in one piece of the arena
uint8_t* take_guarded(Arena& a, size_t bytes) { return a.take<uint8_t>(bytes + RX_GUARD); }

template <typename K>
int run_passes(hipStream_t s, RadixWork& w, uint8_t* const kb[2], uint32_t* const vb[2], int& cur, uint32_t n, int lo_bit, int hi_bit, const SegGeom& sg,
               uint32_t flags, const uint8_t* d_text, uint8_t* d_dig) {
  K* k0 = reinterpret_cast<K*>(kb[0]); K* k1 = reinterpret_cast<K*>(kb[1]);
  const bool noval = vb[0] == nullptr, first = (flags & CJS_RADIX_FIRST_HIST) != 0;
  if constexpr (sizeof(K) == 8) {
    if (flags & CJS_RADIX_GEN) {                  // the segmented sentinel sort of round 1, as sort_round1 (bwt_round1.hip) calls it
      const GenSrc gen{d_text, 0, 7, 0};
      return radix_passes<uint64_t>(s, w, k0, vb[0], k1, vb[1], cur, n, 0, 63, nullptr, &sg, &gen);
    }
  } else {
    if (flags & CJS_RADIX_SEGMENTS) return radix_pass_segments(s, w, k0, vb[0], k1, vb[1], cur, sg.nseg, sg.stride, lo_bit, hi_bit, noval, first);
  }
  return radix_passes<K>(s, w, k0, vb[0], k1, vb[1], cur, n, lo_bit, hi_bit, nullptr, sg.nseg > 1 ? &sg : nullptr, nullptr, noval, first, d_dig);
}

}  // namespace

extern "C" int cjs_stage_radix(const void* keys, int key_bytes, const uint32_t* vals, const uint8_t* text, const uint32_t* first_hist, uint32_t n,
                               int lo_bit, int hi_bit, uint32_t nseg, uint32_t stride, uint32_t n_last, size_t work_cap, uint32_t flags,
                               int work_fill, void* keys_out, uint32_t* vals_out, int* cur_out, uint64_t* guard_bad, const cjs_opts* opts) {
  CJS_GUARD_BEGIN
  CJS_TRY(select_device(opts));
  if (n == 0) return 0;
  const bool gen = flags & CJS_RADIX_GEN, segments = flags & CJS_RADIX_SEGMENTS, with_dig = flags & CJS_RADIX_DIG, with_hist = flags & CJS_RADIX_FIRST_HIST;
  if ((key_bytes != 4 && key_bytes != 8) || lo_bit < 0 || lo_bit >= hi_bit || hi_bit > 8 * key_bytes || (flags & ~RX_FLAGS)) return CJS_E_INVALID_ARG;
  if (nseg == 0 || stride == 0 || n_last == 0 || n_last > stride || (uint64_t)(nseg - 1) * stride + n_last != n) return CJS_E_INVALID_ARG;
  if (nseg == 1 && stride != n) return CJS_E_INVALID_ARG;
  if (work_cap < n || work_cap > RX_MAX_CAP) return CJS_E_INVALID_ARG;
  if (gen && (flags != CJS_RADIX_GEN || key_bytes != 8 || lo_bit != 0 || hi_bit != 63 || !text)) return CJS_E_INVALID_ARG;
  if (segments && (key_bytes != 4 || n_last != stride || with_dig)) return CJS_E_INVALID_ARG;
  if ((!gen && !keys) || (with_hist && !first_hist) || !keys_out || !cur_out || !guard_bad) return CJS_E_INVALID_ARG;
  const bool noval = !gen && !vals;               // generated keys bring their values (the positions) along
  if (!noval && !vals_out) return CJS_E_INVALID_ARG;

  const size_t kb = (size_t)key_bytes;
  const uint8_t fill = (uint8_t)(work_fill & 0xFF);
  const uint32_t tps = ((nseg > 1 ? stride : n) + RS_TILE - 1) / RS_TILE;
  const SegGeom sg{nseg, stride, n_last, tps};
  const size_t T = (size_t)nseg * tps;
  const size_t ht = RadixWork::hist_tiles_for(work_cap), segs = RadixWork::segs_for(work_cap);
  Arena arena;
  // workspace; both key arrays; both value arrays; the byte array; the text (n + 16); take()'s rounding of ten pieces; slack
  CJS_TRY(arena.init(4 * RadixWork::hist_words(ht) + 4 * 256 * segs + 2 * (kb * n + RX_GUARD) + 2 * (4 * (size_t)n + RX_GUARD) + ((size_t)n + RX_GUARD) +
                     ((size_t)n + 16) + 16 * 256 + 65536));
  RadixWork w;
  CJS_TRY(w.carve(arena, ht, segs));
  uint8_t* d_k[2] = {take_guarded(arena, kb * n), take_guarded(arena, kb * n)};
  uint32_t* d_v[2] = {nullptr, nullptr};
  if (!noval) for (int i = 0; i < 2; i++) d_v[i] = reinterpret_cast<uint32_t*>(take_guarded(arena, 4 * (size_t)n));
  uint8_t* d_dig = with_dig ? take_guarded(arena, n) : nullptr;
  uint8_t* d_text = gen ? arena.take<uint8_t>((size_t)n + 16) : nullptr;      // 16 bytes of slack behind the text, as stages.hip carves d_T
  if (!d_k[0] || !d_k[1] || (!noval && (!d_v[0] || !d_v[1])) || (with_dig && !d_dig) || (gen && !d_text)) return CJS_E_OUT_OF_MEMORY;
  // the guarded arrays, for the count behind the run
  struct Guarded { const uint8_t* p; size_t bytes; };
  std::vector<Guarded> guarded = {{d_k[0], kb * n}, {d_k[1], kb * n}};
  if (!noval) { guarded.push_back({reinterpret_cast<uint8_t*>(d_v[0]), 4 * (size_t)n}); guarded.push_back({reinterpret_cast<uint8_t*>(d_v[1]), 4 * (size_t)n}); }
  if (with_dig) guarded.push_back({d_dig, n});

  Stream s;
  CJS_HIP_TRY(hipStreamCreate(s.put()));
  CJS_HIP_TRY(hipMemsetAsync(arena.base, fill, arena.used, s));      // workspace, both buffer pairs, byte array, guards, the text's slack
  if (gen) CJS_HIP_TRY(hipMemcpyAsync(d_text, text, n, hipMemcpyHostToDevice, s));
  else {
    CJS_HIP_TRY(hipMemcpyAsync(d_k[0], keys, kb * n, hipMemcpyHostToDevice, s));
    if (!noval) CJS_HIP_TRY(hipMemcpyAsync(d_v[0], vals, 4 * (size_t)n, hipMemcpyHostToDevice, s));
  }
  // (a geometry with more tiles than the workspace has rows is refused by radix_passes: nothing of it is copied in)
  if (with_hist && T <= w.hist_tiles) CJS_HIP_TRY(hipMemcpyAsync(w.hist, first_hist, 4 * 256 * T, hipMemcpyHostToDevice, s));
  int cur = 0;
  const int rc = key_bytes == 8 ? run_passes<uint64_t>(s, w, d_k, d_v, cur, n, lo_bit, hi_bit, sg, flags, d_text, d_dig)
                                : run_passes<uint32_t>(s, w, d_k, d_v, cur, n, lo_bit, hi_bit, sg, flags, d_text, d_dig);
  std::vector<uint8_t> g(guarded.size() * RX_GUARD);
  for (size_t i = 0; i < guarded.size(); i++)
    CJS_HIP_TRY(hipMemcpyAsync(g.data() + i * RX_GUARD, guarded[i].p + guarded[i].bytes, RX_GUARD, hipMemcpyDeviceToHost, s));
  CJS_HIP_TRY(hipStreamSynchronize(s));
  uint64_t bad = 0;
  for (uint8_t b : g) bad += b != fill;
  *guard_bad = bad;
  if (rc) return rc;
  CJS_HIP_TRY(hipMemcpyAsync(keys_out, d_k[cur], kb * n, hipMemcpyDeviceToHost, s));
  if (!noval) CJS_HIP_TRY(hipMemcpyAsync(vals_out, d_v[cur], 4 * (size_t)n, hipMemcpyDeviceToHost, s));
  CJS_HIP_TRY(hipStreamSynchronize(s));
  *cur_out = cur;
  return 0;
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}
