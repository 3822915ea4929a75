// api.hip — what every entry point of libcjs_hip.so (include/cjs_hip.h) shares: the error detail, the device and pinned-host
// buffer pools, the per-device cache table and what a call reads of cjs_opts.  No CPU fallback: without a HIP device every call
// fails loudly.
#include "cjs_internal.h"
#include "host.h"
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>
#include <mutex>
#include <vector>

using namespace cjs;

// detail text of the last failing call on this thread: the reference's `optDetail` (J/Bzip2_joined_.js:1385-1391)
namespace cjs {
static thread_local char g_detail[192] = {0};
void clear_detail() { g_detail[0] = 0; }
void set_detail(const char* fmt, ...) {
  va_list ap; va_start(ap, fmt);
  vsnprintf(g_detail, sizeof g_detail, fmt, ap);
  va_end(ap);
}
bool env_debug() { static const bool on = getenv("CJS_DEBUG") != nullptr; return on; }
bool env_no_ctx_cache() { static const bool on = getenv("CJS_NO_CTX_CACHE") != nullptr; return on; }
}  // namespace cjs

extern "C" {

const char* cjs_version(void) { return "cjs_hip 0.1 (gfx950)"; }

int cjs_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

void cjs_free(void* p) { cjs::HostPool::give(p); }

const char* cjs_last_error_detail(void) { return g_detail; }

const char* cjs_strerror(int code) {
  switch (code) {
    case CJS_OK: return "ok";
    case CJS_E_NOT_BZIP_DATA: return "Not bzip data";
    case CJS_E_DATA_ERROR: return "Data error";
    case CJS_E_OUT_OF_MEMORY: return "Out of memory";
    case CJS_E_OBSOLETE_INPUT: return "Obsolete (pre 0.9.5) bzip format not supported.";
    case CJS_E_BAD_LEVEL: return "Invalid block size multiplier";
    case CJS_E_BAD_MAGIC: return "Bad magic";
    case CJS_E_NO_DEVICE: return "no HIP device available (this library has no CPU fallback)";
    case CJS_E_HIP: return "HIP runtime error";
    case CJS_E_INVALID_ARG: return "invalid argument";
    case CJS_E_OUTPUT_TOO_SMALL: return "output buffer too small";
    case CJS_E_UNSUPPORTED: return "not supported";
    default: return "unknown error";
  }
}

}  // extern "C"

namespace cjs {

// ---- DevPool and HostPool (see cjs_internal.h): one design, two instances
namespace {
// A table of buffers, each handed out (busy) or cached (idle), keyed by device.  take(): the smallest idle buffer of the key that
// holds the request and is at most twice as large (or any size up to 1 MiB: requests below that are plain allocations of their
// own size class and never claim a big idle buffer), else a new one.  give(): beyond limit() bytes of idle buffers the largest
// idle ones are freed.  Under the lock only the table is edited; buffers are freed after it is released.
struct Pool {
  struct Buf { void* p; size_t bytes; int key; bool busy; };
  void* (*alloc)(size_t bytes, size_t& got);       // a new buffer of got >= bytes bytes, nullptr if none
  void (*release)(const std::vector<Buf>& gone);   // frees buffers that have left the table
  size_t (*limit)();
  std::mutex mu;
  std::vector<Buf> bufs;

  void* take(size_t bytes, int key) {
    {
      std::lock_guard<std::mutex> lock(mu);
      Buf* best = nullptr;
      for (auto& b : bufs)
        if (!b.busy && b.key == key && b.bytes >= bytes && (b.bytes / 2 <= bytes || b.bytes <= ((size_t)1 << 20)) && (!best || b.bytes < best->bytes)) best = &b;
      if (best) { best->busy = true; return best->p; }
    }
    size_t got = 0;
    void* p = alloc(bytes, got);
    if (!p) return nullptr;
    std::lock_guard<std::mutex> lock(mu);
    bufs.push_back(Buf{p, got, key, true});
    return p;
  }
  bool give(void* p) {                              // false: p is not a buffer of the pool
    std::vector<Buf> gone;
    {
      std::lock_guard<std::mutex> lock(mu);
      size_t i = 0;
      while (i < bufs.size() && bufs[i].p != p) i++;
      if (i == bufs.size()) return false;
      bufs[i].busy = false;
      size_t idle = 0;
      for (auto& b : bufs) if (!b.busy) idle += b.bytes;
      while (idle > limit()) {                      // over the limit: the largest idle buffers go first
        size_t big = bufs.size();
        for (size_t k = 0; k < bufs.size(); k++) if (!bufs[k].busy && (big == bufs.size() || bufs[k].bytes > bufs[big].bytes)) big = k;
        if (big == bufs.size()) break;
        idle -= bufs[big].bytes;
        gone.push_back(bufs[big]);
        bufs.erase(bufs.begin() + (long)big);
      }
    }
    if (!gone.empty()) release(gone);
    return true;
  }
  void trim() {                                     // frees every idle buffer
    std::vector<Buf> gone;
    {
      std::lock_guard<std::mutex> lock(mu);
      for (size_t i = 0; i < bufs.size();) {
        if (bufs[i].busy) { i++; continue; }
        gone.push_back(bufs[i]);
        bufs.erase(bufs.begin() + (long)i);
      }
    }
    if (!gone.empty()) release(gone);
  }
};

size_t env_mb(const char* name, size_t dflt) { const char* e = getenv(name); return (e ? (size_t)strtoull(e, nullptr, 10) : dflt) << 20; }

// device buffers: hipMalloc, keyed by device.  CJS_DEVICE_POOL_MB (default 65536) of idle buffers per process; none under
// CJS_NO_CTX_CACHE (give() frees at once).  A failed hipMalloc trims the pool and tries once more.
Pool g_dev{
    [](size_t bytes, size_t& got) -> void* {
      void* p = nullptr;
      if (hipMalloc(&p, bytes) != hipSuccess) {
        DevPool::trim();                            // cached-but-idle buffers may be what is in the way
        if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
      }
      got = bytes;
      return p;
    },
    [](const std::vector<Pool::Buf>& gone) {        // each on its own device; the caller's device is restored
      int cur = 0;
      const bool have = hipGetDevice(&cur) == hipSuccess;
      for (auto& b : gone) if (hipSetDevice(b.key) == hipSuccess) (void)hipFree(b.p);
      if (have) (void)hipSetDevice(cur);
    },
    [] { static const size_t lim = env_no_ctx_cache() ? 0 : env_mb("CJS_DEVICE_POOL_MB", 65536); return lim; }};

// pinned result buffers: portable (every GPU of a multi-device call copies into them), 1/16 larger than asked for (a later result
// of about the same size fits too), CJS_PINNED_RESULT_MB (default 2048) of idle buffers
Pool g_host{
    [](size_t bytes, size_t& got) -> void* {
      void* p = nullptr;
      got = bytes + bytes / 16;
      if (hipHostMalloc(&p, got, hipHostMallocPortable) != hipSuccess || !p) { (void)hipGetLastError(); return nullptr; }
      return p;
    },
    [](const std::vector<Pool::Buf>& gone) { for (auto& b : gone) (void)hipHostFree(b.p); },
    [] { static const size_t lim = env_mb("CJS_PINNED_RESULT_MB", 2048); return lim; }};
}  // namespace

void* DevPool::take(size_t bytes) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  return g_dev.take(bytes ? bytes : 4, dev);
}
void DevPool::give(void* p) { if (p && !g_dev.give(p)) (void)hipFree(p); }      // not ours: a plain buffer
void DevPool::trim() { g_dev.trim(); }

void* HostPool::take(size_t bytes) {
  if (!bytes) bytes = 1;
  void* p = bytes < ((size_t)1 << 20) || !g_host.limit() ? nullptr : g_host.take(bytes, 0);
  return p ? p : malloc(bytes);                                                    // small, unpinned by setting, or pinning failed
}
void HostPool::give(void* p) { if (p && !g_host.give(p)) free(p); }              // not pinned: plain malloc
void HostPool::trim() { g_host.trim(); }

Opts::Opts(const cjs_opts* o) {
  if (o && o->struct_size >= sizeof(cjs_opts)) { device = o->device; n_devices = o->n_devices; flags = o->flags; stats = o->stats; }
  if (const char* e = getenv("CJS_DEVICES")) n_devices = (uint32_t)atoi(e);
}

int select_device(const cjs_opts* opts) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return CJS_E_NO_DEVICE;
  const int dev = Opts(opts).device;
  if (dev >= n) return CJS_E_INVALID_ARG;
  if (dev >= 0) CJS_HIP_TRY(hipSetDevice(dev));
  return 0;
}

int current_device(const cjs_opts* opts, int& dev) {
  CJS_TRY(select_device(opts));
  int ndev = 0, cur = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || hipGetDevice(&cur) != hipSuccess) return CJS_E_NO_DEVICE;
  dev = cur;
  return 0;
}

static DevCache g_cache[MAX_DEVICES][CACHE_SLOTS];      // per-device context caches (host.h)
DevCache& dev_cache(int device, int slot) { return g_cache[device][slot]; }

}  // namespace cjs
