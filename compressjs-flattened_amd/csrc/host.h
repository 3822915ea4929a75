// host.h — host-side plumbing of the entry points (definitions in api.hip): what a call reads of cjs_opts, the per-device
// context caches, scoped DevPool buffers and worker threads.
#pragma once
#include "cjs_internal.h"
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <mutex>
#include <thread>
#include <vector>

namespace cjs {

// What a call reads of its cjs_opts; a struct smaller than this library's cjs_opts (an older caller) counts as none.  CJS_DEVICES,
// when set, overrides n_devices (JS / Python callers shard without an opts struct); each caller clamps n_devices its own way.
struct Opts {
  int device = -1;                 // -1: the current device
  uint32_t n_devices = 0, flags = 0;
  cjs_stats* stats = nullptr;
  explicit Opts(const cjs_opts* o);
};
int select_device(const cjs_opts* opts);      // makes opts' device current; CJS_E_NO_DEVICE without any
int current_device(const cjs_opts* opts, int& dev);      // select_device, then dev = the device that is current now

// Per-device cache of a context and its device staging buffers, kept between host-buffer calls.  Slots of a device:
//   0 .. SHARD_SLOTS-1  cjs_bzip2_compress: slot 0 the one-GPU call and the first shard of a multi-GPU call on the device, the
//                       others the further shards on the same device (more shards than GPUs)
//   BOUNDARY_SLOT       the boundary pass of a multi-GPU / chunked cjs_bzip2_compress (device 0)
//   BATCH_SLOT          cjs_bzip2_compress_batch.  Never slot 0: the batch call holds its slot while it passes an input above
//                       BATCH_GROUP_BYTES to cjs_bzip2_compress, which takes slot 0 (one mutex for both would deadlock).
constexpr int MAX_DEVICES = 64, SHARD_SLOTS = 4, BOUNDARY_SLOT = SHARD_SLOTS, BATCH_SLOT = BOUNDARY_SLOT + 1, CACHE_SLOTS = BATCH_SLOT + 1;
struct DevCache {
  std::mutex mu;
  cjs_ctx* ctx = nullptr;
  DevMem<uint8_t> d_in, d_out;
  size_t in_cap = 0, out_cap = 0;
  void release() {
    cjs_ctx_destroy(ctx);
    ctx = nullptr; d_in.reset(); d_out.reset(); in_cap = out_cap = 0;
  }
  // Device buffer `buf` of `cap` bytes made to hold `need`; never shrinks.  keep = false: the contents go, exactly `need` bytes
  // (failure: buf empty); keep = true: the contents are copied on stream s into max(need, 1.5 cap) + 4096 bytes (failure: unchanged).
  static int grow(DevMem<uint8_t>& buf, size_t& cap, size_t need, bool keep = false, hipStream_t s = nullptr) {
    if (buf && need <= cap) return 0;
    if (!keep) {
      cap = 0;
      CJS_TRY(buf.alloc(need));
      cap = need;
      return 0;
    }
    const size_t to = std::max(need, cap + cap / 2) + 4096;
    DevMem<uint8_t> p;
    CJS_HIP_TRY(hipMalloc((void**)p.put(), to));
    if (buf && (hipMemcpyAsync(p, buf, cap, hipMemcpyDeviceToDevice, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)) return CJS_E_HIP;
    buf = std::move(p); cap = to;
    return 0;
  }
};
DevCache& dev_cache(int device, int slot);     // device < MAX_DEVICES, slot < CACHE_SLOTS

// A cache slot's mutex, held for one call.  At scope exit the slot is released if the call failed (check(rc) / drop(): after an
// error the cached state is not trusted) or CJS_NO_CTX_CACHE is set.
struct CacheLease {
  DevCache& c;
  std::lock_guard<std::mutex> lock{c.mu};
  bool dropped = env_no_ctx_cache();
  ~CacheLease() { if (dropped) c.release(); }
  int check(int rc) { if (rc) dropped = true; return rc; }
  void drop() { dropped = true; }
};

// One DevPool buffer, given back when its owner goes or at reset().
struct PoolGive { void operator()(void* p) const { DevPool::give(p); } };
struct DevBuf : Owner<void*, PoolGive> {
  explicit DevBuf(size_t bytes) { p = DevPool::take(bytes); }
};

// One HostPool buffer (or malloc'd memory: reset(p) adopts it), given back when its owner goes; release() hands it to the caller.
// Where a share's stream copies into or out of it, it is declared in front of the share: given back once that stream has drained.
struct HostGive { void operator()(void* p) const { HostPool::give(p); } };
struct HostBuf : Owner<uint8_t*, HostGive> {
  HostBuf() = default;
  explicit HostBuf(size_t bytes) { p = (uint8_t*)HostPool::take(bytes); }
  uint8_t* release() { uint8_t* q = p; p = nullptr; return q; }
};

// v's bytes as a result of the C ABI: malloc'd (the caller frees it with cjs_free), *out / *out_n set; on failure both are left alone
inline int malloc_result(const std::vector<uint8_t>& v, uint8_t** out, size_t* out_n) {
  uint8_t* host = (uint8_t*)malloc(v.size() ? v.size() : 1);
  if (!host) return CJS_E_OUT_OF_MEMORY;
  if (!v.empty()) memcpy(host, v.data(), v.size());
  *out = host; *out_n = v.size();
  return 0;
}

// Device d made current at scope exit (the caller's device, restored on every path out).
struct RestoreDevice {
  int d;
  ~RestoreDevice() { (void)hipSetDevice(d); }
};
// The device of a call: select() makes opts' device current (current_device); from then on it is made current again at scope exit.
struct CallDevice {
  int dev = -1;
  int select(const cjs_opts* opts) { return current_device(opts, dev); }
  ~CallDevice() { if (dev >= 0) (void)hipSetDevice(dev); }
};

// f(), an exception that leaves it turned into rc (std::bad_alloc: CJS_E_OUT_OF_MEMORY, else CJS_E_HIP); rc untouched otherwise
template <typename F> void guarded(int& rc, F&& f) noexcept {
  try { f(); }
  catch (const std::bad_alloc&) { rc = CJS_E_OUT_OF_MEMORY; }
  catch (...) { rc = CJS_E_HIP; }
}
// Worker threads, joined on every path out of the scope that started them.  run(rc, f): f() on a thread of its own, under
// guarded(rc, f) (nothing may leave a thread: std::terminate).
struct Workers {
  std::vector<std::thread> th;
  ~Workers() { join(); }
  template <typename F> void run(int& rc, F f) { th.emplace_back([&rc, f] { guarded(rc, f); }); }
  void join() { for (auto& t : th) t.join(); th.clear(); }
};

}  // namespace cjs
