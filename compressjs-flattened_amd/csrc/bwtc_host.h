// bwtc_host.h — host logic of BWTC.compressFile (J/BWTC_joined_.js:1698-1825): the serial range coder with its two-thread
// split, the framing in front of the coder (stream head, block heads) and the plan that cuts a job's blocks into batches.  No HIP
// in here (tests/host/bwtc_host_check.cc compiles it with the host compiler and runs it under the sanitizers).
#pragma once
#include "bwtc_format.h"
#include <pthread.h>
#include <sched.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <mutex>
#include <thread>
#include <vector>

namespace cjs {
namespace {      // internal linkage, as when this stood in bwtc.hip: the library exports none of it

// RangeCoder encode side (J/BWTC_joined_.js:40-153).  The interval arithmetic is one serial chain over the whole file, but it
// is TWO chains: `range` never depends on `low` (range' = f(range, step); low only receives r * lt and is shifted when range is).
// In split mode (default) the calling thread runs the range chain alone and leaves one record per step -- the addend r * lt and
// the number of byte shifts in front of it -- in a ring of buffers; a second host thread replays them on `low` (carry
// propagation, pending 0xFF bytes, output).  Same bytes as the one-thread form (CJS_BWTC_SPLIT_CODER=0), which runs both
// chains in one loop at ~5 ns per step.
struct HostCoder {
  std::vector<uint8_t>& out;                            // bytes [0, len) are output; the vector is kept larger (reserve())
  static constexpr uint32_t RING = 8, RCAP = 1u << 15;
  std::vector<uint64_t> ring[RING];
  uint32_t ring_n[RING];
  int ring_cpu[RING];
  std::thread low_thread;
  // the two threads of the split mode write their own state at every step: each side on cache lines of its own (with range
  // and low on one line the pair ran 8x slower than one thread)
  alignas(128) uint8_t* data = nullptr;                 // ---- low side
  size_t len = 0;
  uint32_t low = 0, help = 0, bytecount = 0;
  int buffer = 0;
  alignas(128) uint32_t range = 0x80000000u;            // ---- range side
  bool split = false;
  uint64_t* cur = nullptr;
  uint32_t cur_n = 0;
  alignas(128) std::atomic<uint64_t> produced{0};       // written by the range side
  alignas(128) std::atomic<uint64_t> consumed{0};       // written by the low side
  alignas(128) std::atomic<bool> closing{false};
  std::atomic<bool> failed{false};                      // the low thread ran out of memory (it keeps draining the ring)
  uint64_t dbg_full_spins = 0;                          // range side: polls while the ring was full (CJS_DEBUG)
  alignas(128) uint64_t dbg_empty_spins = 0;            // low side: polls while the ring was empty
  int dbg_low_cpu[2] = {-1, -1};
  int near_cpu = -1;                                    // low side: the cpu the range side was last seen on
  cpu_set_t allowed;                                    // the caller's affinity when the split started
  bool have_allowed = false;
  explicit HostCoder(std::vector<uint8_t>& o) : out(o) { len = o.size(); reserve(4096); }
  ~HostCoder() { stop_thread(); }
  void reserve(size_t extra) {                          // room for `extra` more bytes (a coder step emits at most 3)
    if (len + extra > out.size()) out.resize(std::max(out.size() * 2, len + extra));
    data = out.data();
  }
  void reserve_steps(size_t nsteps) { if (!split) reserve(3 * nsteps + help + 4096); }      // (split mode: the low thread reserves per buffer)
  inline void emit(uint8_t b) { data[len++] = b; }
  void start(int c, uint32_t initlen) { low = 0; range = 0x80000000u; buffer = c; help = 0; bytecount = initlen; }
  // one byte shift of the low chain: what leaves (or stays pending) is decided by low alone
  inline void shift_low() {
    if (low < (0xFFu << 23)) { emit((uint8_t)buffer); for (; help; help--) emit(0xFF); buffer = (low >> 23) & 0xFF; }
    else if (low & 0x80000000u) { emit((uint8_t)(buffer + 1)); for (; help; help--) emit(0x00); buffer = (low >> 23) & 0xFF; }
    else help++;
    low = (low << 8) & 0x7FFFFFFFu; bytecount++;
  }
  inline void normalize() {
    while (range <= 0x00800000u) { shift_low(); range <<= 8; }
  }
  // normalize() for the step loop: whether a byte leaves is a coin flip per step, so the usual case (at most one
  // byte, no pending carry bytes, no carry) is written without a branch: unconditional store, conditional advance
  inline void normalize_step() {
    const uint32_t need = range <= 0x00800000u;
    if (__builtin_expect((range <= 0x00008000u) | (need & (uint32_t)((low >= (0xFFu << 23)) | (help != 0))), 0)) { normalize(); return; }
    data[len] = (uint8_t)buffer;
    len += need;
    buffer = need ? (int)((low >> 23) & 0xFF) : buffer;
    low = need ? (low << 8) & 0x7FFFFFFFu : low;
    range = need ? range << 8 : range;
    bytecount += need;
  }
  // ---- split mode, range side (calling thread)
  void start_split() {
    for (auto& r : ring) r.assign(RCAP, 0ull);
    cur = ring[0].data(); cur_n = 0; split = true;
    have_allowed = sched_getaffinity(0, sizeof allowed, &allowed) == 0;
    near_cpu = sched_getcpu();
    low_thread = std::thread([this] { low_loop(); });
    keep_off_my_core(low_thread);
  }
  // Where the second thread runs decides what the split is worth (2-socket EPYC host of the MI355X box, 100 MB): on another core
  // of the caller's L3 domain 169-200 ms of coding, elsewhere on the caller's socket 200-225 ms, on the OTHER socket 310-360 ms
  // (every ring line the range side writes was last read over there: slower than one thread, 308 ms), on the caller's own core
  // (its second hardware thread) ~320 ms.  So the low thread's affinity is set to the CPUs that share the caller's L3 minus the
  // caller's core; if that cannot be read, to the caller's package minus its core; if that cannot be read either, nothing is
  // changed.  The caller's own affinity is never touched.  CJS_BWTC_NO_AFFINITY=1 switches this off.
  static bool read_cpu_list(const char* fmt, int cpu, cpu_set_t* set) {
    char path[128];
    snprintf(path, sizeof path, fmt, cpu);
    FILE* f = fopen(path, "r");
    if (!f) return false;
    char line[512] = {0};
    const bool ok = fgets(line, sizeof line, f) != nullptr;
    fclose(f);
    if (!ok) return false;
    CPU_ZERO(set);
    int n = 0;
    for (char* p = line; *p;) {                          // "a,b-c,d" lists
      char* e = nullptr;
      const long a = strtol(p, &e, 10);
      if (e == p) break;
      long b2 = a;
      if (*e == '-') { p = e + 1; b2 = strtol(p, &e, 10); }
      for (long c = a; c <= b2 && c < CPU_SETSIZE; c++) if (c >= 0) { CPU_SET((int)c, set); n++; }
      if (*e != ',') break;
      p = e + 1;
    }
    return n > 0;
  }
  void keep_off_my_core(std::thread& t) { place_near(t.native_handle(), sched_getcpu()); }
  void place_near(pthread_t th, int cpu) {        // th: the low thread; cpu: where the range side runs
    static const bool off = getenv("CJS_BWTC_NO_AFFINITY") != nullptr;
    if (off || cpu < 0) return;
    cpu_set_t mine, near;
    if (!read_cpu_list("/sys/devices/system/cpu/cpu%d/topology/thread_siblings_list", cpu, &mine)) return;
    if (!have_allowed) return;
    const char* domains[2] = {"/sys/devices/system/cpu/cpu%d/cache/index3/shared_cpu_list", "/sys/devices/system/cpu/cpu%d/topology/package_cpus_list"};
    for (const char* d : domains) {
      if (!read_cpu_list(d, cpu, &near)) continue;
      cpu_set_t want;
      CPU_ZERO(&want);
      int left = 0;
      for (int c = 0; c < CPU_SETSIZE; c++) if (CPU_ISSET(c, &near) && CPU_ISSET(c, &allowed) && !CPU_ISSET(c, &mine)) { CPU_SET(c, &want); left++; }
      if (left > 0) { (void)pthread_setaffinity_np(th, sizeof want, &want); return; }
    }
  }
  inline uint32_t shifts_needed() {                     // (zero or one shift is a coin flip per step: no branch for it)
    if (__builtin_expect(range <= 0x00008000u, 0)) { uint32_t k = 0; while (range <= 0x00800000u) { range <<= 8; k++; } return k; }
    const uint32_t k = range <= 0x00800000u;
    range <<= (k << 3);
    return k;
  }
  inline void push(uint32_t add, uint32_t k) {
    cur[cur_n++] = (uint64_t)add | ((uint64_t)k << 32);
    if (cur_n == RCAP) hand_over();
  }
  void hand_over() {                                    // the full (or last) buffer goes to the low thread
    const uint64_t p = produced.load(std::memory_order_relaxed);
    ring_n[p % RING] = cur_n;
    ring_cpu[p % RING] = sched_getcpu();                 // (the low thread follows this thread when the scheduler moves it)
    produced.store(p + 1, std::memory_order_release);
    while (p + 1 - consumed.load(std::memory_order_acquire) >= RING) { __builtin_ia32_pause(); dbg_full_spins++; }
    cur = ring[(p + 1) % RING].data(); cur_n = 0;
  }
  // ---- split mode, low side (its own thread): replays (shifts, addend) on low
  void low_loop() {
    dbg_low_cpu[0] = sched_getcpu();
    for (;;) {
      dbg_low_cpu[1] = sched_getcpu();
      const uint64_t c = consumed.load(std::memory_order_relaxed);
      uint32_t spins = 0;
      while (produced.load(std::memory_order_acquire) == c) {
        if (closing.load(std::memory_order_acquire) && produced.load(std::memory_order_acquire) == c) return;
        __builtin_ia32_pause();                          // (a polling loop without it starves the other hardware thread of the core)
        dbg_empty_spins++;
        if (++spins > 4096) { std::this_thread::yield(); spins = 0; }
      }
      const uint64_t* rec = ring[c % RING].data();
      uint32_t n = ring_n[c % RING];
      if (ring_cpu[c % RING] != near_cpu) { near_cpu = ring_cpu[c % RING]; if (c) place_near(pthread_self(), near_cpu); }      // the range side moved
      if (!failed.load(std::memory_order_relaxed)) {
        try { reserve(4 * (size_t)n + help + 64); } catch (...) { failed.store(true, std::memory_order_relaxed); }
      }
      if (failed.load(std::memory_order_relaxed)) n = 0;
      for (uint32_t i = 0; i < n; i++) {
        const uint64_t e = rec[i];
        uint32_t k = (uint32_t)(e >> 32);
        // the usual case without a branch, as in normalize_step(): at most one shift, no pending bytes, no carry
        const uint32_t need = k;
        if (__builtin_expect((k > 1u) | ((k != 0u) & (uint32_t)((low >= (0xFFu << 23)) | (help != 0))), 0)) { for (; k; k--) shift_low(); }
        else {
          data[len] = (uint8_t)buffer;
          len += need;
          buffer = need ? (int)((low >> 23) & 0xFF) : buffer;
          low = need ? (low << 8) & 0x7FFFFFFFu : low;
          bytecount += need;
        }
        low += (uint32_t)e;
      }
      consumed.store(c + 1, std::memory_order_release);
    }
  }
  void stop_thread() {
    if (!low_thread.joinable()) return;
    if (cur_n) hand_over();
    closing.store(true, std::memory_order_release);
    low_thread.join();
    split = false;
  }
  inline void freq(uint32_t sy, uint32_t lt, uint32_t tot) {
    if (split) { const uint32_t k = shifts_needed(); const uint32_t r = range / tot, tmp = r * lt; range = (lt + sy < tot) ? r * sy : range - tmp; push(tmp, k); return; }
    normalize();
    const uint32_t r = range / tot, tmp = r * lt;
    low += tmp;
    if (lt + sy < tot) range = r * sy; else range -= tmp;
  }
  // same arithmetic with the division replaced by a multiply with a 64-bit reciprocal: the quotient sits on the serial
  // (low, range) chain, the reciprocal (looked up by tot, which comes from the step list) does not
  inline void freq_rcp(uint32_t sy, uint32_t lt, uint32_t tot, const uint64_t* rcp) {
    // rcp[tot] = floor(2^64 / tot) + 1: the high half of range * rcp is floor(range / tot) exactly (range < 2^32, tot < 2^17:
    // range * (rcp*tot - 2^64) < 2^49 < 2^64), so no correction step sits on the chain
    if (split) {
      const uint32_t k = shifts_needed();
      const uint32_t r = (uint32_t)(((unsigned __int128)range * rcp[tot]) >> 64), tmp = r * lt;
      range = (lt + sy < tot) ? r * sy : range - tmp;
      push(tmp, k);
      return;
    }
    normalize_step();
    const uint32_t r = (uint32_t)(((unsigned __int128)range * rcp[tot]) >> 64);
    const uint32_t tmp = r * lt;
    low += tmp;
    range = (lt + sy < tot) ? r * sy : range - tmp;
  }
  inline void shift(uint32_t sy, uint32_t lt, int sh) {
    if (split) { const uint32_t k = shifts_needed(); const uint32_t r = range >> sh, tmp = r * lt; range = ((lt + sy) >> sh) ? range - tmp : r * sy; push(tmp, k); return; }
    normalize();
    const uint32_t r = range >> sh, tmp = r * lt;
    low += tmp;
    if ((lt + sy) >> sh) range -= tmp; else range = r * sy;
  }
  void finish() {
    if (split) { const uint32_t k = shifts_needed(); push(0u, k); stop_thread(); }      // the closing normalisation as a record; then the low side is ours again
    reserve(help + 16);
    normalize();
    bytecount += 5;
    uint32_t tmp = low >> 23;
    if ((low & 0x7FFFFFu) >= ((bytecount & 0xFFFFFFu) >> 1)) tmp++;
    if (tmp > 0xFF) { emit((uint8_t)(buffer + 1)); for (; help; help--) emit(0x00); }
    else { emit((uint8_t)buffer); for (; help; help--) emit(0xFF); }
    emit((uint8_t)(tmp & 0xFF));
    emit((uint8_t)((bytecount >> 16) & 0xFF)); emit((uint8_t)((bytecount >> 8) & 0xFF)); emit((uint8_t)(bytecount & 0xFF));
    out.resize(len);
  }
};
// reciprocals floor(2^64 / tot) + 1 for every total a step can carry (17 bits); tot < 2 keeps the division
inline const uint64_t* rcp_table() {
  static std::vector<uint64_t> rcp;
  static std::once_flag rcp_once;
  std::call_once(rcp_once, [] { rcp.assign(1u << 17, 0ull); for (uint32_t t = 2; t < (1u << 17); t++) rcp[t] = (uint64_t)(((unsigned __int128)1 << 64) / t) + 1; });
  return rcp.data();
}
// the serial tail: one list of model steps through the coder.  The compressor's block loop and cjs_stage_bwtc_code
// both run THIS loop (always inlined: the compressor's copy is the loop it had in place)
__attribute__((always_inline)) inline void code_steps(HostCoder& coder, const uint64_t* steps, uint32_t ns, const uint64_t* rc_tab) {
  for (uint32_t i = 0; i < ns; i++) {
    const uint64_t st = steps[i];
    const Step s = unpack(st);
    if (st & STEP_SHIFT_FLAG) coder.shift(s.sy, s.lt, (int)s.tot);
    else if (s.tot >= 2) coder.freq_rcp(s.sy, s.lt, s.tot, rc_tab);
    else coder.freq(s.sy, s.lt, s.tot);
  }
}
inline void nomodel(HostCoder& c, int bits, uint32_t sym) { for (int i = bits - 1; i >= 0; i--) c.shift(1, (sym >> i) & 1, 1); }   // :1281-1287
inline void logdist(HostCoder& c, int block_size, uint32_t d) {                                                                   // :1241-1253
  const int lb = lgbits(block_size);
  if (d < 2) { nomodel(c, lb, d); return; }
  const int lg = fls32(d);
  nomodel(c, lb, (uint32_t)lg);
  nomodel(c, lg - 1, d & ((1u << (lg - 1)) - 1));
}

// ---------------------------------------------------------------- framing
// The magic and writeUnsignedNumber(size + 1) (:605-620) but for the number's last byte, which is returned: the coder starts
// with it (:1700).  W1: a stream without .size gives varint(0).
inline int write_stream_head(std::vector<uint8_t>& out, size_t n, bool size_unknown) {
  out.push_back('b'); out.push_back('w'); out.push_back('t'); out.push_back('c');
  uint8_t vb[12]; int nv = 0;
  uint64_t v = size_unknown ? 0 : (uint64_t)n + 1;
  do { vb[nv++] = (uint8_t)(v & 0x7F); v >>= 7; } while (v);
  vb[0] |= 0x80;
  for (int i = nv - 1; i >= 1; i--) out.push_back(vb[i]);
  return vb[0];
}
// What a block codes in front of its model section (:1734-1765): full or short with the length, the primary index, and which
// of the 256 byte values it holds (alist[0, asz), any order) as the use-tree.
inline void code_block_head(HostCoder& coder, uint32_t bs, uint32_t length, uint32_t pidx, const uint8_t* alist, uint32_t asz) {
  if (length == bs) coder.freq(1, 0, 3);                         // "full size block" :1734
  else { coder.freq(1, 1, 3); logdist(coder, (int)bs, length); } // "short block" :1737-1738
  logdist(coder, (int)bs, pidx);                                 // :1742
  uint16_t tree[512]; memset(tree, 0, sizeof tree);              // use-tree :1744-1765
  for (uint32_t i = 0; i < asz; i++) tree[256 + alist[i]] = 1;
  for (int i = 255; i > 0; i--) tree[i] = (uint16_t)(tree[2 * i] + tree[2 * i + 1]);
  tree[0] = 1;
  for (int i = 1; i < 512; i++) {
    const int parent = i >> 1, full = use_tree_full(i);
    if (tree[parent] == 0 || tree[parent] == full * 2) continue;
    if (i >= 256) coder.shift(1, tree[i] ? 1 : 0, 1);
    else coder.freq(1, tree[i] == 0 ? 0u : tree[i] == full ? 2u : 1u, 3);
  }
}

// ---------------------------------------------------------------- batch plan
// Blocks are dealt to the device slots in contiguous ranges (cjs_opts.n_devices / CJS_DEVICES; SURVEY §8e "BWTC compress":
// replicable stages x N, serial tail x 1), each range cut into batches of at most BWTC_MAX_BATCH blocks; the first batch of the
// job is small (first_batch blocks, 0 = no such rule) so that the coder starts early.
constexpr uint32_t BWTC_FIRST_BATCH = 8, BWTC_MAX_BATCH = 512;
struct BatchPlan {
  int slot = 0, device = 0, seq = 0;          // seq: order of the batch inside its slot
  uint32_t first = 0, count = 0;
};
inline uint32_t plan_slots(uint32_t n_devices, uint32_t nb) { return std::max(1u, std::min(std::min(n_devices, 64u), nb)); }
// nslots = plan_slots(..): slot sl runs on device sl mod ndev, a lone slot on the caller's device dev0
inline std::vector<BatchPlan> plan_batches(uint32_t nb, uint32_t nslots, int ndev, int dev0, uint32_t first_batch) {
  std::vector<BatchPlan> plan;
  const uint32_t share = (nb + nslots - 1) / nslots;
  for (uint32_t sl = 0; sl < nslots; sl++) {
    uint32_t k = std::min<uint32_t>(sl * share, nb);
    const uint32_t end = std::min<uint32_t>(k + share, nb);
    int seq = 0;
    while (k < end) {
      uint32_t c = std::min<uint32_t>(end - k, BWTC_MAX_BATCH);
      if (sl == 0 && seq == 0 && first_batch && end - k > 2 * first_batch) c = first_batch;      // the coder starts on this one (doubling batches behind it: no gain, 232-243 ms either way)
      BatchPlan B;
      B.slot = (int)sl; B.device = nslots == 1 ? dev0 : (int)(sl % (uint32_t)ndev); B.seq = seq++; B.first = k; B.count = c;
      plan.push_back(B);
      k += c;
    }
  }
  return plan;
}

}  // namespace
}  // namespace cjs
