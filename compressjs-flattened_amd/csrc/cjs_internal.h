// cjs_internal.h — shared host-side declarations of the HIP library (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <stdio.h>
#include <new>
#include "cjs_hip.h"
#include "bwt_rules.h"      // bits_for, enum Counter

#define CJS_HIP_TRY(expr)                                                                   \
  do {                                                                                      \
    hipError_t _e = (expr);                                                                 \
    if (_e != hipSuccess) {                                                                 \
      fprintf(stderr, "[cjs_hip] %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
      return _e == hipErrorOutOfMemory ? CJS_E_OUT_OF_MEMORY : CJS_E_HIP;                    \
    }                                                                                       \
  } while (0)
#define CJS_TRY(expr) do { int _rc = (expr); if (_rc) return _rc; } while (0)

namespace cjs {

// thread-local detail text behind cjs_last_error_detail() (api.hip)
void clear_detail();
void set_detail(const char* fmt, ...);
// read from the environment once per process (api.hip): CJS_DEBUG (timings and decisions on stderr), CJS_NO_CTX_CACHE
bool env_debug(); bool env_no_ctx_cache();

// Body of an extern "C" entry point: C++ exceptions (std::bad_alloc from a container fed by untrusted sizes) never
// cross the C ABI, they become return codes.
#define CJS_GUARD_BEGIN try {
#define CJS_GUARD_END(oom_value, other_value)                          \
  } catch (const std::bad_alloc&) { return (oom_value); }              \
  catch (...) { return (other_value); }

// Move-only owner of one HIP handle or allocation; null is empty.  The destructor and reset() release it with Free.  Releasing
// never synchronises and never changes the current device: a caller that needs either does it first.
template <typename T, typename Free> struct Owner {
  T p = nullptr;
  Owner() = default;
  Owner(Owner&& o) noexcept : p(o.p) { o.p = nullptr; }
  Owner& operator=(Owner&& o) noexcept { if (this != &o) { reset(o.p); o.p = nullptr; } return *this; }
  ~Owner() { reset(); }
  void reset(T v = nullptr) { if (p) Free{}(p); p = v; }
  T* put() { reset(); return &p; }          // for the call that creates it: hipStreamCreate(s.put())
  operator T() const { return p; }
  T operator->() const { return p; }
};
struct StreamFree { void operator()(hipStream_t s) const { (void)hipStreamDestroy(s); } };
struct EventFree { void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); } };
struct PinnedFree { void operator()(void* p) const { (void)hipHostFree(p); } };
struct DevFree { void operator()(void* p) const { (void)hipFree(p); } };
using Stream = Owner<hipStream_t, StreamFree>;
using Event = Owner<hipEvent_t, EventFree>;
template <typename T> using Pinned = Owner<T*, PinnedFree>;   // hipHostMalloc
template <typename T> struct DevMem : Owner<T*, DevFree> {    // hipMalloc
  int alloc(size_t bytes) {
    if (hipMalloc((void**)this->put(), bytes) == hipSuccess) return 0;
    this->p = nullptr;
    return CJS_E_OUT_OF_MEMORY;
  }
};

struct DevPool;
// simple device arena: one hipMalloc (or one buffer of the per-device pool), bump allocation, 256-byte aligned; freed by its owner
struct Arena {
  uint8_t* base = nullptr;
  size_t cap = 0, used = 0;
  bool pooled = false;
  Arena() = default;
  Arena(const Arena&) = delete;
  Arena& operator=(const Arena&) = delete;
  ~Arena() { destroy(); }
  int init(size_t bytes) {
    CJS_HIP_TRY(hipMalloc((void**)&base, bytes));
    cap = bytes; used = 0; pooled = false;
    return 0;
  }
  inline int init_pooled(size_t bytes);      // from DevPool: kept between calls (cjs_trim / CJS_NO_CTX_CACHE give it back)
  inline void destroy();
  template <typename T> T* take(size_t n) {
    size_t bytes = (n * sizeof(T) + 255) & ~(size_t)255;
    if (used + bytes > cap) return nullptr;
    T* p = (T*)(base + used);
    used += bytes;
    return p;
  }
};

struct EventTimer {   // accumulates device time of bracketed regions on one stream
  hipStream_t s = nullptr;
  Event a, b;
  int init(hipStream_t st) { s = st; CJS_HIP_TRY(hipEventCreate(a.put())); CJS_HIP_TRY(hipEventCreate(b.put())); return 0; }
  void start() { (void)hipEventRecord(a, s); }
  double stop() { (void)hipEventRecord(b, s); (void)hipEventSynchronize(b); float ms = 0; (void)hipEventElapsedTime(&ms, a, b); return ms; }
};

// Per-device cache of device buffers for the host-buffer entry points (hipMalloc / hipFree of the multi-GB scratch of
// one call cost milliseconds): take() hands out the smallest cached free buffer that is large enough or allocates one,
// give() returns it to the cache, trim() frees everything cached (cjs_trim; CJS_NO_CTX_CACHE=1 makes give() free at once).
struct DevPool {
  static void* take(size_t bytes);
  static void give(void* p);
  static void trim();
};
// Result buffers handed to the caller by the host-buffer entry points ("malloc'd by the library; release with cjs_free").
// Large results come from a cache of PINNED host buffers: the device-to-host copy of the result is then one DMA at link speed
// into pages that exist already, instead of a staged copy into fresh pageable memory that faults page by page (100 MB:
// ~20 ms).  cjs_free() returns such a buffer to the cache (at most CJS_PINNED_RESULT_MB of idle buffers are kept, default
// 2048; 0 = results are plain malloc), cjs_trim() frees the idle ones.  Small results are plain malloc.
struct HostPool {
  static void* take(size_t bytes);      // never pinned below 1 MiB; falls back to malloc when pinning fails
  static void give(void* p);            // any pointer take() returned (or malloc'd memory)
  static void trim();
};
inline int Arena::init_pooled(size_t bytes) {
  base = (uint8_t*)DevPool::take(bytes);
  if (!base) return CJS_E_OUT_OF_MEMORY;
  cap = bytes; used = 0; pooled = true;
  return 0;
}
inline void Arena::destroy() {
  if (base) { if (pooled) DevPool::give(base); else (void)hipFree(base); }
  base = nullptr; cap = used = 0;
}

constexpr uint32_t RS_TILE = 4096;   // radix-sort tile (256 threads x 16 keys)

// Workspace of the radix sorter (radix.hip): room for sorts of up to hist_tiles tiles in up to bintot_segs segments.  The rest of
// the code relies on two things: hist is free between sorts (sort_round of bwt.hip borrows it as hcount), and the chunk sums of
// the long-segment scan sit behind the hist_tiles per-tile rows (hist_words counts them in).
struct RadixWork {
  uint32_t* hist = nullptr;      // hist_words(hist_tiles): 256 per tile (tile-major) + the chunk sums
  uint32_t* bintot = nullptr;    // 256 per segment
  uint32_t hist_tiles = 0, bintot_segs = 0;
  // sizes for sorting up to `cap` keys: segmented sorts round every segment up to whole tiles, one extra tile per 64 Ki keys
  static size_t hist_tiles_for(size_t cap) { return (cap + RS_TILE - 1) / RS_TILE + cap / 65536 + 258; }
  static size_t segs_for(size_t cap) { return cap / 65536 + 2; }
  static size_t hist_words(size_t tiles) { return 256 * (tiles + tiles / 64 + 2); }
  int carve(Arena& a, size_t tiles, size_t segs);
};
struct LaunchTimes {   // event pairs around the dominant kernel; resolved after the stream has drained
  static constexpr int MAXP = 512;
  hipEvent_t ev[2 * MAXP];
  uint64_t elems[MAXP];
  int n = 0, made = 0;
  bool enabled = false, open = false;
  uint64_t min_elems = 0;          // only launches over at least this many elements are timed (the full-size passes of a sort)
  void begin(hipStream_t s, uint64_t e) {
    open = false;
    if (!enabled || n >= MAXP || e < min_elems) return;
    open = true;
    while (made < 2 * (n + 1)) { if (hipEventCreate(&ev[made]) != hipSuccess) { enabled = false; open = false; return; } made++; }
    elems[n] = e;
    (void)hipEventRecord(ev[2 * n], s);
  }
  void end(hipStream_t s) { if (!enabled || !open || n >= MAXP) return; (void)hipEventRecord(ev[2 * n + 1], s); n++; open = false; }
  void resolve(cjs_stats* st) {
    double ms = 0; uint64_t e = 0;
    for (int i = 0; i < n; i++) { float t = 0; if (hipEventElapsedTime(&t, ev[2 * i], ev[2 * i + 1]) == hipSuccess) { ms += t; e += elems[i]; } }
    if (st && n) { st->ms_bwt_dominant = ms / n; st->bwt_dominant_launches = (uint64_t)n; st->bwt_dominant_bytes = e; }
    reset();
  }
  void reset() { for (int i = 0; i < made; i++) (void)hipEventDestroy(ev[i]); n = made = 0; }
  ~LaunchTimes() { reset(); }
  // hands the recorded launches to `to` (appended; this object is left empty, still enabled)
  void move_into(LaunchTimes& to) {
    for (int i = 0; i < n && to.n < MAXP; i++) {
      if (to.made > 2 * to.n) { for (int j = 2 * to.n; j < to.made; j++) (void)hipEventDestroy(to.ev[j]); to.made = 2 * to.n; }
      to.ev[2 * to.n] = ev[2 * i]; to.ev[2 * to.n + 1] = ev[2 * i + 1]; to.elems[to.n] = elems[i]; to.n++; to.made = 2 * to.n;
    }
    for (int i = 2 * n; i < made; i++) (void)hipEventDestroy(ev[i]);
    n = made = 0;
  }
};

struct SegGeom; struct GenSrc;      // radix.hpp
// LSD radix passes over n keys (with their values unless noval) between k0 / v0 and k1 / v1, one per 8-bit digit from lo_bit up
// while the digit starts below hi_bit: the word sorted on is bits [lo_bit, lo_bit + 8 * ceil((hi_bit - lo_bit) / 8)), clipped at
// the key width -- WHOLE digits.  A caller whose hi_bit - lo_bit is no multiple of 8 gets the sort on [lo_bit, hi_bit) only if the
// rest of the last digit is equal in all keys of a segment (every such caller says why at its call; tests/test_gpu_radix.py
// holds the rule).  n > 0.  cur says which pair holds the keys, before and after.  seg: sorted as segments (else one); gen: the
// first pass makes its keys from the block bytes.  Instantiated for K = uint64_t and uint32_t.
template <typename K>
int radix_passes(hipStream_t s, RadixWork& w, K* k0, uint32_t* v0, K* k1, uint32_t* v1, int& cur, uint32_t n, int lo_bit, int hi_bit,
                 LaunchTimes* lt = nullptr, const SegGeom* seg = nullptr, const GenSrc* gen = nullptr, bool noval = false,
                 bool first_hist_ready = false, uint8_t* dig = nullptr);
// The five phase-1 passes of the packed cyclic round 1 (bytes 6..2 of every suffix, keys made from the block bytes gen.T): 8-byte
// records through k0 / k1 for two passes, then the narrow records of bwt_rules.h through n0 / n1; sorted, they end in n0.
// dig: a byte per key
int radix_passes_pk1(hipStream_t s, RadixWork& w, uint64_t* k0, uint64_t* k1, uint32_t* n0, uint32_t* n1, uint32_t n, LaunchTimes* lt,
                     const SegGeom& sg, const GenSrc& gen, uint8_t* dig);
// ... over nseg segments of `stride` 32-bit keys each (dec_ibwt.hip: one segment per block)
int radix_pass_segments(hipStream_t s, RadixWork& w, uint32_t* k0, uint32_t* v0, uint32_t* k1, uint32_t* v1, int& cur, uint32_t nseg, uint32_t stride,
                        int lo_bit, int hi_bit, bool noval, bool first_hist_ready);

// Workspace of the suffix sorter for up to `cap` suffixes (all blocks of a batch together).
struct BwtWork {
  size_t cap = 0;
  uint64_t* key[2] = {nullptr, nullptr};
  uint32_t* val[2] = {nullptr, nullptr};
  uint32_t* pos[2] = {nullptr, nullptr};
  uint8_t* ghead = nullptr;      // per slot of a round >= 2, in front of the sort: 1 = the slot starts a group (the regroup before wrote it)
  uint32_t* R = nullptr;
  uint32_t* SA = nullptr;
  uint8_t* dflag = nullptr;      // per slot of a round >= 2: 1 = its group is too large for the tile sorters
  uint8_t* hflag = nullptr;      // per slot of a round >= 2, behind the sort: bit 0 = head of the new grouping, bit 1 = head of the previous one
  RadixWork rs;                  // of the radix passes
  uint32_t* tile_cnt = nullptr;  // 3 * tiles (+ scanned copies)
  uint32_t* counters = nullptr;  // 16, of which five are in use: see enum Counter in bwt_rules.h
  Pinned<uint32_t> h_counters;     // host mirror
  Event ev_scan;                   // recorded behind the tile scan of a round (the host waits for the counters, not for the round)
  LaunchTimes lt;                  // dominant-kernel events of the last bwt_run that was given a stats struct
  static size_t bytes_needed(size_t cap);
  int carve(Arena& a, size_t cap);
};

// Suffix-sorts nb blocks (block k = d_T[k*stride .. +n_k), n_k = stride except the last = n_last)
// and writes the BWT bytes to d_U (same layout) and the primary indices to d_pidx[nb].
int bwt_run(hipStream_t s, BwtWork& w, const uint8_t* d_T, uint32_t nb, uint32_t stride, uint32_t n_last,
            bool cyclic, uint8_t* d_U, uint32_t* d_pidx, cjs_stats* stats, bool resolve_stats = true);
// Cyclic form over nb blocks of DIFFERENT lengths (a batch of independent inputs): block k = d_T[k*stride .. +d_len[k]),
// 1 <= d_len[k] <= stride (device array); BWT bytes to d_U with the same layout.  The slots past a block's length are ignored.
int bwt_run_var(hipStream_t s, BwtWork& w, const uint8_t* d_T, uint32_t nb, uint32_t stride, const uint32_t* d_len,
                uint8_t* d_U, uint32_t* d_pidx);
// Inverse sentinel BWT of nb blocks back to back in d_T (lengths lens[], primary indices pidx[], host arrays) into d_out (dec_ibwt.hip)
int ibwt_sentinel_run(hipStream_t s, const uint8_t* d_T, uint32_t max_len, uint32_t nb, const uint32_t* lens, const uint32_t* pidx, uint8_t* d_out);
// BWTC model evaluation of nb blocks (bwtc_model.hip): one workgroup per block, DefSumModel (fast, levels 1-5) or FenwickModel
// (levels 6-9); reads mb.A / a_stride / asz / npos (mtf.h), leaves block k's coder steps at d_steps + k * step_stride, their count in d_nsteps[k]
struct MtfBufs;
int bwtc_model_launch(hipStream_t s, bool fast, const MtfBufs& mb, uint32_t nb, uint64_t* d_steps, size_t step_stride, uint32_t* d_nsteps);

}  // namespace cjs
