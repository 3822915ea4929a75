// enc_host.hip — cjs_bzip2_compress: the host-buffer driver of the compress pipeline (pipeline.hip).  One GPU and an input below
// CJS_CHUNK_BYTES: the cached context of the device, upload, cjs_bzip2_compress_device, download.  Several GPUs and / or a very
// large input: contiguous block ranges on per-GPU worker threads (compress_multi).  cjs_bzip2_compress_indexed is the same call with
// the rows of every block handed up to the calling thread (enc_index.h).  Also cjs_trim.
#include "ctx.h"
#include "host.h"
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <vector>

using namespace cjs;

// The context of cache slot `hc` (host.h) for n input bytes at `level` on the CURRENT device (range_blocks as in
// cjs_ctx_create_sharded), staging buffers of at least in_bytes / out_bytes (0 = not needed).  Grows, never shrinks.
static int ensure(DevCache& hc, size_t n, int level, long range_blocks, size_t in_bytes, size_t out_bytes) {
  const cjs_ctx* c = hc.ctx;
  if (!c || c->level != level || c->max_input < n || (range_blocks ? c->range_blocks != (size_t)range_blocks : c->range_blocks != c->max_blocks)) {
    cjs_ctx_destroy(hc.ctx); hc.ctx = nullptr;
    CJS_TRY(cjs_ctx_create_sharded(&hc.ctx, -1, n, range_blocks, level));
  }
  if (in_bytes) CJS_TRY(DevCache::grow(hc.d_in, hc.in_cap, in_bytes));
  if (out_bytes) CJS_TRY(DevCache::grow(hc.d_out, hc.out_cap, out_bytes));
  return 0;
}

// One shard of a multi-GPU job: its own device, context and stream.  A shard is a run of consecutive blocks; because the
// RLE1 state is fresh at every block start, the input bytes [start(first), start(first + count)) form a
// stream of their own whose blocks are exactly those blocks, so a shard uploads and processes ONLY its byte range.
// All shards at once (one per GPU): the shards meet once -- every shard publishes (bit length, CRC fold) of its blocks -- and
// then pack at their FINAL bit offset; their fragments are disjoint runs of whole words of the stream and go from the device
// straight to their place in the result buffer (no merge pass).  In waves (more ranges than may run at a time: very large
// inputs): a shard packs from bit 0 and keeps its bytes, the host shifts them into place at the end.
struct MultiSync {                       // the one meeting of the shards of a call
  std::mutex mu;
  std::condition_variable cv;
  uint32_t published = 0, nshards = 0;
  int rc = 0;                            // first failure of any shard: everyone stops
  std::vector<cjs_shard_meta> metas;
  uint8_t* out = nullptr;                // result buffer, allocated by the coordinating thread once the length is known
  bool out_ready = false;
  void publish(uint32_t i, const cjs_shard_meta& m, int shard_rc) {
    std::lock_guard<std::mutex> lock(mu);
    metas[i] = m;
    if (shard_rc && !rc) rc = shard_rc;
    published++;
    cv.notify_all();
  }
};
struct Shard {
  int device = 0, slot = 0, rc = 0;
  uint32_t index = 0;
  long first = 0, count = 0;
  uint64_t byte_lo = 0, byte_hi = 0;
  const uint8_t* d_resident = nullptr;   // the range is already in this device's memory (the boundary pass put it there)
  uint64_t bits = 0;
  std::vector<uint8_t> bytes;            // wave mode: the shard's bit string from bit 0
  uint32_t crc_fold = 0;
  bool want_rows = false;                // an indexed call: the rows of the shard's blocks (its bytes are a stream of their own, so
  EncRowsWant rows;                      // they are complete), set at the shard's bit offset by the calling thread
  EncRowsWant* want() { return want_rows ? &rows : nullptr; }
};
// What an indexed call collects on the calling thread: the entries and counts of the whole stream, its last block's end.
struct HostTables {
  bool lines = false;
  std::vector<cjs_bz_index_entry> entries;
  std::vector<uint32_t> newlines;
  uint64_t end_bit = ENC_FIRST_BIT;
  void append(const EncRowsWant& w, uint64_t start_bit, int level) { end_bit = enc_rows_append(entries, newlines, w.rows.data(), w.rows.size(), start_bit, level); }
};
static void run_shard_body(Shard* sh, const uint8_t* in, int level, MultiSync* sync, bool& published) {
  if (hipSetDevice(sh->device) != hipSuccess) { sh->rc = CJS_E_HIP; return; }
  const size_t n = (size_t)(sh->byte_hi - sh->byte_lo);
  const size_t per = (size_t)sh->count * ((size_t)level * 100000);
  const size_t out_cap = (per + per / 4 + 65536 + 3) & ~(size_t)3;
  DevCache local;                                                        // shards beyond the cached slots of a device: a context of their own
  CacheLease hc{sh->slot < BOUNDARY_SLOT ? dev_cache(sh->device, sh->slot) : local};
  if (sh->slot >= BOUNDARY_SLOT) hc.drop();
  if ((sh->rc = hc.check(ensure(hc.c, n, level, 0, sh->d_resident ? 0 : (n ? n : 4), out_cap))) != 0) return;
  cjs_ctx* c = hc.c.ctx;
  const uint8_t* d_in = sh->d_resident ? sh->d_resident : hc.c.d_in;
  if (!sh->d_resident && n && hipMemcpyAsync(hc.c.d_in, in + sh->byte_lo, n, hipMemcpyHostToDevice, c->stream) != hipSuccess) { sh->rc = CJS_E_HIP; hc.drop(); return; }
  if (env_debug()) fprintf(stderr, "[cjs] shard %u on device %d (slot %d): blocks [%ld, %ld), bytes [%llu, %llu): H2D %zu B%s\n", sh->index, sh->device, sh->slot, sh->first, sh->first + sh->count,
                           (unsigned long long)sh->byte_lo, (unsigned long long)sh->byte_hi, sh->d_resident ? (size_t)0 : n, sh->d_resident ? " (resident from the boundary pass)" : "");
  if (!sync) {                                                           // wave mode: bare bit string from bit 0
    long total = 0;
    std::vector<uint32_t> crcs((size_t)sh->count + 1, 0u);
    sh->rc = compress_core(c, d_in, n, level, 0, -1, false, hc.c.d_out, out_cap, &sh->bits, crcs.data(), (long)crcs.size(), &total, nullptr, sh->want());
    if (!sh->rc && total != sh->count) sh->rc = CJS_E_HIP;          // cannot happen: the range was cut at block starts
    if (!sh->rc) {
      for (long k = 0; k < sh->count; k++) sh->crc_fold = crc_fold(sh->crc_fold, crcs[(size_t)k]);
      sh->bytes.resize((size_t)((sh->bits + 7) / 8) + 16);
      if (hipMemcpy(sh->bytes.data(), hc.c.d_out, sh->bytes.size(), hipMemcpyDeviceToHost) != hipSuccess) sh->rc = CJS_E_HIP;
    }
    hc.check(sh->rc);
    return;
  }
  cjs_shard_meta meta{};
  sh->rc = shard_blocks_impl(c, d_in, n, level, 0, 1, nullptr, &meta, nullptr, sh->want());      // the byte range is a stream of its own
  if (!sh->rc && (long)meta.total_blocks != sh->count) sh->rc = CJS_E_HIP;           // cannot happen: the range was cut at block starts
  sync->publish(sh->index, meta, sh->rc);
  published = true;
  if (drain_on_error(c, sh->rc)) { hc.drop(); return; }
  {
    std::unique_lock<std::mutex> lk(sync->mu);
    sync->cv.wait(lk, [&] { return sync->out_ready || sync->rc; });
    if (sync->rc) { c->sh_state = 0; return; }
  }
  uint64_t start, total; uint32_t scrc; int writer;
  shard_layout(sync->metas.data(), (int)sync->nshards, (int)sh->index, start, total, scrc, writer);
  if (!meta.blocks && sh->index) { c->sh_state = 0; return; }
  size_t fo = 0, fl = 0; uint64_t so = 0;
  sh->rc = shard_pack_core(c, level, sh->index == 0, (int)sh->index == writer, start, meta.bits, scrc, hc.c.d_out, out_cap, &fo, &fl, &so);
  c->sh_state = 0;
  if (!sh->rc && fl && hipMemcpy(sync->out + so, hc.c.d_out + fo, fl, hipMemcpyDeviceToHost) != hipSuccess) sh->rc = CJS_E_HIP;
  hc.check(sh->rc);
}
static void run_shard(Shard* sh, const uint8_t* in, int level, MultiSync* sync) {
  bool published = false;
  if (sh->count == 0) { if (sync) sync->publish(sh->index, cjs_shard_meta{}, 0); return; }      // no blocks: nothing of the stream comes from here
  guarded(sh->rc, [&] { run_shard_body(sh, in, level, sync, published); });     // (after an exception too, the others hear of it below)
  if (sync && !published) sync->publish(sh->index, cjs_shard_meta{}, sh->rc ? sh->rc : CJS_E_HIP);
  if (sync && sh->rc) { std::lock_guard<std::mutex> lock(sync->mu); if (!sync->rc) sync->rc = sh->rc; sync->cv.notify_all(); }
}

// Multi-GPU host path: ONE boundary pass over the stream (device 0: the input start of every block),
// then blocks are dealt in contiguous ranges to per-GPU worker threads, each of which gets only its byte range; the only
// cross-shard data are (bit length, CRC fold).  Contexts and staging buffers are kept per device between calls.  The steps:

// boundary pass: the input start of every block of the whole stream, and n behind them (device 0, slot `bc`; its copy of the input
// serves the shards that run there)
static int block_starts(CacheLease& bc, const uint8_t* in, size_t n, int level, std::vector<uint64_t>& starts) {
  CJS_HIP_TRY(hipSetDevice(0));
  int rc = ensure(bc.c, n, level, 1, n ? n : 4, 0);
  uint32_t nbk = 0;
  if (!rc && hipMemcpyAsync(bc.c.d_in, in, n, hipMemcpyHostToDevice, bc.c.ctx->stream) != hipSuccess) rc = CJS_E_HIP;
  if (!rc) rc = rle1_run(bc.c.ctx->stream, bc.c.ctx->rle, bc.c.d_in, n, &nbk);
  std::vector<RleBlock> hb(nbk);
  if (!rc && nbk && hipMemcpy(hb.data(), bc.c.ctx->rle.blocks, sizeof(RleBlock) * nbk, hipMemcpyDeviceToHost) != hipSuccess) rc = CJS_E_HIP;
  CJS_TRY(bc.check(rc));
  starts.resize((size_t)nbk + 1);
  for (uint32_t k = 0; k < nbk; k++) starts[k] = hb[k].s;
  starts[nbk] = n;
  return 0;
}
// the blocks dealt in contiguous ranges, range i on device i % ndev; d_in0: device 0's copy of the whole input
static std::vector<Shard> deal_ranges(const std::vector<uint64_t>& starts, uint32_t nshards, int ndev, bool waves, const uint8_t* d_in0) {
  const long total = (long)starts.size() - 1;
  const long share = total ? (total + nshards - 1) / nshards : 0;
  std::vector<Shard> sh(nshards);
  for (uint32_t i = 0; i < nshards; i++) {
    sh[i].index = i;
    sh[i].device = (int)(i % (uint32_t)ndev);
    sh[i].slot = waves ? 0 : (int)(i / (uint32_t)ndev);          // shards that share a device at the same time need contexts of their own
    sh[i].first = std::min<long>((long)i * share, total);
    sh[i].count = std::min<long>(share, total - sh[i].first);
    sh[i].byte_lo = starts[(size_t)sh[i].first]; sh[i].byte_hi = starts[(size_t)(sh[i].first + sh[i].count)];
    if (sh[i].device == 0) sh[i].d_resident = d_in0 + sh[i].byte_lo;
  }
  return sh;
}
// all ranges at once: they meet at `sync`, where this thread allocates the result once its length is known
static int run_all_at_once(std::vector<Shard>& sh, const uint8_t* in, int level, uint8_t** out, size_t* out_n, HostTables* tables) {
  const uint32_t nshards = (uint32_t)sh.size();
  MultiSync sync;
  sync.nshards = nshards; sync.metas.assign(nshards, cjs_shard_meta{});
  HostBuf result; size_t len = 0;
  {
    Workers workers;
    for (uint32_t i = 0; i < nshards; i++) workers.run(sh[i].rc, [&, i] { run_shard(&sh[i], in, level, &sync); });
    std::unique_lock<std::mutex> lk(sync.mu);
    sync.cv.wait(lk, [&] { return sync.published == nshards; });
    if (!sync.rc) {
      uint64_t start, tbits; uint32_t scrc; int writer;
      shard_layout(sync.metas.data(), (int)nshards, 0, start, tbits, scrc, writer);
      len = (size_t)((tbits + 80 + 7) / 8);
      result.reset((uint8_t*)HostPool::take(len));
      if (!result) sync.rc = CJS_E_OUT_OF_MEMORY;
      sync.out = result; sync.out_ready = true;
    }
    sync.cv.notify_all();
  }                                                           // (joined)
  int rc = sync.rc;
  for (auto& x : sh) if (x.rc && !rc) rc = x.rc;
  if (rc) return rc;
  if (tables) {                                               // every shard's rows at the bit its first block stands at
    std::vector<uint64_t> at(nshards);
    uint64_t start, tbits; uint32_t scrc; int writer;
    shard_layout(sync.metas.data(), (int)nshards, 0, start, tbits, scrc, writer, at.data());
    for (uint32_t i = 0; i < nshards; i++) if (!sh[i].rows.rows.empty()) tables->append(sh[i].rows, at[i], level);
    if (tables->end_bit != tbits) return CJS_E_HIP;
  }
  *out = result.release(); *out_n = len;
  return 0;
}
// max_parallel ranges at a time, each a bare bit string from bit 0; then the stitch: header, the strings shifted to their place
// (interiors by a few threads: disjoint whole bytes; then the shared end bytes one range after the other), trailer
static int run_in_waves(std::vector<Shard>& sh, const uint8_t* in, int level, uint32_t max_parallel, uint8_t** out, size_t* out_n, HostTables* tables) {
  const uint32_t nshards = (uint32_t)sh.size();
  for (uint32_t i0 = 0; i0 < nshards; i0 += max_parallel) {
    Workers workers;
    for (uint32_t i = i0; i < nshards && i < i0 + max_parallel; i++) workers.run(sh[i].rc, [&, i] { run_shard(&sh[i], in, level, nullptr); });
  }
  std::vector<cjs_shard_meta> metas(nshards, cjs_shard_meta{});
  for (uint32_t i = 0; i < nshards; i++) {
    if (sh[i].rc) return sh[i].rc;
    metas[i].bits = sh[i].bits; metas[i].blocks = (uint32_t)sh[i].count; metas[i].crc_fold = sh[i].crc_fold;
  }
  std::vector<uint64_t> at(nshards);
  uint64_t start, total; uint32_t scrc; int writer;
  shard_layout(metas.data(), (int)nshards, 0, start, total, scrc, writer, at.data());
  const size_t len = (size_t)((total + 80 + 7) / 8);
  if (tables) {
    for (uint32_t i = 0; i < nshards; i++) if (!sh[i].rows.rows.empty()) tables->append(sh[i].rows, at[i], level);
    if (tables->end_bit != total) return CJS_E_HIP;
  }
  HostBuf o;
  o.reset((uint8_t*)calloc(len + 16, 1));                      // (plain malloc'd memory: what cjs_free gives back to free())
  if (!o) return CJS_E_OUT_OF_MEMORY;
  o.p[0] = 'B'; o.p[1] = 'Z'; o.p[2] = 'h'; o.p[3] = (uint8_t)('0' + level);
  const uint32_t nt = std::min<uint32_t>(nshards, 8u);
  std::vector<int> mrc(nt, 0);
  {
    Workers mergers;
    for (uint32_t t = 0; t < nt; t++) mergers.run(mrc[t], [&, t] { for (uint32_t i = t; i < nshards; i += nt) if (sh[i].bits) funnel_merge(o.p, at[i], sh[i].bytes.data(), sh[i].bits, 0); });
  }
  for (int r : mrc) if (r) return r;
  for (uint32_t i = 0; i < nshards; i++) if (sh[i].bits) funnel_merge(o.p, at[i], sh[i].bytes.data(), sh[i].bits, 1);
  put_trailer(o.p, total, scrc);
  *out = o.release(); *out_n = len;
  return 0;
}
// max_parallel = shards in flight at a time (0 = all): one at a time bounds the workspace when the ranges are only there to
// cut a very large input into pieces (each piece's workspace is ~70 B per byte of its blocks)
static int compress_multi(const uint8_t* in, size_t n, int level, uint32_t nshards, uint8_t** out, size_t* out_n, uint32_t max_parallel, HostTables* tables) {
  int ndev = 0, dev0 = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || hipGetDevice(&dev0) != hipSuccess) return CJS_E_NO_DEVICE;
  if (ndev > MAX_DEVICES) ndev = MAX_DEVICES;
  RestoreDevice restore{dev0};
  CacheLease bc{dev_cache(0, BOUNDARY_SLOT)};
  std::vector<uint64_t> starts;
  CJS_TRY(block_starts(bc, in, n, level, starts));
  const bool waves = max_parallel && max_parallel < nshards;
  std::vector<Shard> sh = deal_ranges(starts, nshards, ndev, waves, bc.c.d_in);
  if (tables) for (Shard& x : sh) { x.want_rows = true; x.rows.lines = tables->lines; }
  return waves ? run_in_waves(sh, in, level, max_parallel, out, out_n, tables) : run_all_at_once(sh, in, level, out, out_n, tables);
}

// the body of cjs_bzip2_compress; tables (null: the plain call) collects the rows of an indexed call
static int compress_host(const uint8_t* in, size_t n, int level, uint8_t** out, size_t* out_n, const cjs_opts* opts, HostTables* tables) {
  CJS_TRY(select_device(opts));
  const Opts o(opts);
  uint32_t nshards = o.n_devices;
  {
    // several GPUs and / or a very large input: contiguous block ranges.  With more ranges than devices (inputs above
    // CJS_CHUNK_BYTES, default 2 GiB, are cut so that a range's workspace stays bounded) the ranges run in waves of one per device.
    static const size_t chunk = getenv("CJS_CHUNK_BYTES") ? (size_t)strtoull(getenv("CJS_CHUNK_BYTES"), nullptr, 10) : ((size_t)2 << 30);
    if (nshards > 64) nshards = 64;
    const size_t pieces = (chunk && n > chunk) ? (n + chunk / 2 - 1) / (chunk / 2 ? chunk / 2 : 1) : 0;
    if (n > 0 && (nshards > 1 || pieces > 1)) {
      const uint32_t par = nshards > 1 ? nshards : 1;
      const uint32_t ranges = (uint32_t)std::max<size_t>(par, std::min<size_t>(pieces, 4096));
      return compress_multi(in, n, level, ranges, out, out_n, ranges > par ? par : 0, tables);
    }
  }
  // The workspace (~70 B per input byte), the staging buffers and the streams are kept per device between calls
  // (creating and freeing them costs more than compressing 100 MB); cjs_trim() or CJS_NO_CTX_CACHE=1 gives them back.
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEVICES) return CJS_E_HIP;
  CacheLease hc{dev_cache(dev, 0)};
  const size_t out_cap = (n + n / 4 + 4096 + 3) & ~(size_t)3;
  const bool dbg = env_debug();
  auto now = [] { return std::chrono::steady_clock::now(); };
  auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
  const auto t0 = now();
  CJS_TRY(hc.check(ensure(hc.c, n, level, 0, n ? n : 4, out_cap)));
  cjs_ctx* c = hc.c.ctx;
  const auto t1 = now();
  int rc = 0;
  if (n && hipMemcpyAsync(hc.c.d_in, in, n, hipMemcpyHostToDevice, c->stream) != hipSuccess) rc = CJS_E_HIP;
  if (dbg && !rc) (void)hipStreamSynchronize(c->stream);
  const auto t2 = now();
  size_t len = 0;
  c->stage_times = !(o.flags & CJS_FLAG_NO_STAGE_TIMES);
  EncRowsWant want;
  if (tables) want.lines = tables->lines;
  uint64_t bits = 0;
  if (!rc) rc = compress_core(c, hc.c.d_in, n, level, 0, -1, true, hc.c.d_out, out_cap, &bits, nullptr, 0, nullptr, o.stats, tables ? &want : nullptr);
  len = (size_t)((bits + 7) / 8);
  if (!rc && tables) { tables->append(want, ENC_FIRST_BIT, level); if (tables->end_bit + 80 != bits) rc = CJS_E_HIP; }
  const auto t3 = now();
  uint8_t* host = nullptr;
  if (!rc) { host = (uint8_t*)HostPool::take(len ? len : 1); if (!host) rc = CJS_E_OUT_OF_MEMORY; }
  if (!rc && hipMemcpy(host, hc.c.d_out, len, hipMemcpyDeviceToHost) != hipSuccess) rc = CJS_E_HIP;
  const auto t4 = now();
  if (dbg) fprintf(stderr, "[cjs] host compress: workspace %.2f ms, H2D %.2f ms, pipeline %.2f ms, malloc + D2H %.2f ms\n", ms(t0, t1), ms(t1, t2), ms(t2, t3), ms(t3, t4));
  if (hc.check(rc)) { HostPool::give(host); return rc; }
  *out = host; *out_n = len;
  return 0;
}

extern "C" int cjs_bzip2_compress(const uint8_t* in, size_t n, int level, uint8_t** out, size_t* out_n, const cjs_opts* opts) {
  if (!out || !out_n) return CJS_E_INVALID_ARG;
  *out = nullptr; *out_n = 0;
  clear_detail();
  if (level < 1 || level > 9) return CJS_E_BAD_LEVEL;                 // J/Bzip2_joined_.js:2208
  CJS_GUARD_BEGIN
  return compress_host(in, n, level, out, out_n, opts, nullptr);
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

extern "C" int cjs_bzip2_compress_indexed(const uint8_t* in, size_t n, int level, uint8_t** out, size_t* out_n, cjs_bz_index** idx, cjs_bz_lines** lines,
                                          const cjs_opts* opts) {
  if (out) *out = nullptr;
  if (out_n) *out_n = 0;
  if (idx) *idx = nullptr;
  if (lines) *lines = nullptr;
  if (!out || !out_n || !idx) return CJS_E_INVALID_ARG;
  clear_detail();
  if (level < 1 || level > 9) return CJS_E_BAD_LEVEL;
  CJS_GUARD_BEGIN
  HostTables tables;
  tables.lines = lines != nullptr;
  HostBuf stream; size_t len = 0;
  {
    uint8_t* p = nullptr;
    CJS_TRY(compress_host(in, n, level, &p, &len, opts, &tables));
    stream.reset(p);
  }
  CJS_TRY(enc_tables_make(tables.entries, tables.newlines, tables.end_bit, idx, lines));
  *out = stream.release(); *out_n = len;
  return 0;
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

extern "C" void cjs_trim(void) {
  int cur = 0;
  const bool have = hipGetDevice(&cur) == hipSuccess;
  for (int d = 0; d < MAX_DEVICES; d++)             // (first: the batch contexts' workspaces go back to the DevPool, emptied next)
    for (int k = 0; k < CACHE_SLOTS; k++) {
      DevCache& dc = dev_cache(d, k);
      std::lock_guard<std::mutex> lock(dc.mu);
      if ((dc.ctx || dc.d_in || dc.d_out) && hipSetDevice(d) == hipSuccess) dc.release();
    }
  if (have) (void)hipSetDevice(cur);
  DevPool::trim();
  HostPool::trim();
}
