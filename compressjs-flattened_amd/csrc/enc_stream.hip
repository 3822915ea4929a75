// enc_stream.hip — streaming Bzip2 compression (cjs_bzip2_enc_*): the input arrives in pieces of any size, the .bz2 stream
// leaves in pieces, and the memory an encoder holds depends on its chunk size and level, not on the bytes written.
//
// The RLE1 state is fresh at every block start, so the input from a block's first byte onward, taken as a stream of
// its own, yields exactly that block and its successors.  A step therefore works on `carry + new bytes`: the boundary pass
// (rle1_run) finds nb blocks, all but the last go through the tables and the packer, and the input from the last block's start
// becomes the next carry.  The last block is always held back, even when it is full: only finish() knows that nothing follows
// (Q3: no empty block is ever emitted).  A step that finds no complete block only grows the carry -- a block can swallow ~51
// times its capacity of input (runs of 255 become 5 bytes).
//
// Bits: the packer writes a step's blocks at the bit phase the stream stands at (0..7 bits into a byte; it zeroes the bits in
// front), the host ORs the partial byte it held back from the previous step into the step's first byte and holds back the new
// partial byte.  Nothing is shifted.  The stream CRC is folded over the block CRCs on the host: c = rol1(c) ^ crc.
//
// Threads and streams: write() copies into one of two pinned staging chunks and blocks only when both are full.  One worker
// thread per encoder owns a context of its own (never a dev_cache slot) and runs the steps.  Uploads (staging chunk -> device
// staging chunk) and downloads (packed bytes -> host buffer of the output queue) go on a copy stream: the upload of chunk k + 1
// is issued before step k's kernels, the download of step k is collected during step k + 1.
//
// Output queue: a step's bytes enter the queue only when the queue is empty, or while the caller waits for the worker (in a write
// that found both staging chunks full, or in finish) and so cannot read.  Until then they stay in the worker's one download
// buffer and the worker waits.  A caller that drains after each write of at most chunk_bytes therefore never finds more than one
// step's output; finish adds at most the steps still under way: the one coming down, the one in work, the one staged, the final one.
//
// Index (CJS_FLAG_ENC_INDEX / _LINES): a step's blocks hand their rows (enc_index.h) down with the block CRCs, and the
// worker appends them as entries at the stream's absolute bit, a 64-bit count kept beside the 0..7 phase.  The held-back last block
// is not among a step's cnt blocks, so it is counted once: by the step that packs it.  36 bytes of host memory per block.
#include "cjs_internal.h"
#include "ctx.h"
#include "host.h"
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <thread>

using namespace cjs;

namespace {
constexpr size_t ENC_DEFAULT_CHUNK = (size_t)64 << 20;
constexpr size_t ENC_MIN_CHUNK = (size_t)64 << 10, ENC_MAX_CHUNK = (size_t)1 << 30;

struct Slot {                            // one pinned staging chunk
  Pinned<uint8_t> h;
  size_t n = 0;
  bool full = false, final = false, uploaded = false;
};
struct Piece { uint8_t* p; size_t len, off; };      // HostPool buffer of the output queue
struct Flag {                            // true for a scope (under the encoder's mutex at both ends)
  bool& f;
  explicit Flag(bool& b) : f(b) { f = true; }
  ~Flag() { f = false; }
};
}  // namespace

struct cjs_bz_enc {
  int level = 0, device = -1;
  size_t chunk = 0;
  std::mutex mu;
  std::condition_variable cv;
  int rc = 0;                            // first failure: every later call returns it
  bool started = false, ready = false, finished = false, worker_done = false, quit = false;
  bool writing = false, finishing = false;      // the caller is inside write / finish
  Slot slot[2];
  uint32_t wslot = 0;                    // the slot write() fills
  std::deque<Piece> outq;
  size_t pending = 0;
  std::thread worker;
  // the tables of the stream being written (flags): the worker's until worker_done, read by cjs_bzip2_enc_index after it
  uint32_t flags = 0;
  std::vector<cjs_bz_index_entry> ix_entries;
  std::vector<uint32_t> ix_newlines;
  uint64_t ix_end_bit = ENC_FIRST_BIT;
  int fail(int code) { if (!rc) rc = code; return rc; }      // (mu held)
  // the caller waits for the worker and cannot read meanwhile (mu held)
  bool caller_waits() const { return finishing || (writing && slot[wslot].full); }
};

namespace {

// The worker's side of an encoder: every device resource lives and dies on the worker thread, with its device current.
struct EncWork {
  cjs_bz_enc* e;
  cjs_ctx* ctx = nullptr;
  uint32_t cap = 0, rb = 0;              // block capacity; most blocks a step can take
  DevMem<uint8_t> d_in, d_stage[2], d_out[2];
  size_t in_cap = 0, out_cap = 0;
  Stream cs;                             // copy stream
  Event ev_up[2], ev_dn;
  Pinned<uint32_t> h_crc;
  Pinned<RleBlock> h_blk;
  size_t carry = 0;
  uint32_t scrc = 0, phase = 0, steps = 0, packs = 0;
  uint64_t bit_at = ENC_FIRST_BIT;       // the stream's absolute bit behind the blocks packed so far (an indexing encoder)
  bool header_done = false;
  uint8_t hold = 0;                      // the stream's partial last byte (phase bits), not yet handed out
  // download in flight
  uint8_t* dl = nullptr; size_t dl_len = 0; uint32_t dl_end_phase = 0; bool dl_final = false;

  explicit EncWork(cjs_bz_enc* enc) : e(enc) {}
  ~EncWork() {
    if (ctx) for (hipStream_t s : {ctx->side.p, ctx->tail.p, ctx->stream.p}) if (s) (void)hipStreamSynchronize(s);
    if (cs) (void)hipStreamSynchronize(cs);
    HostPool::give(dl);
    cjs_ctx_destroy(ctx);
  }

  int make_ctx() {
    if (ctx) {
      for (hipStream_t s : {ctx->side.p, ctx->tail.p, ctx->stream.p}) if (s) CJS_HIP_TRY(hipStreamSynchronize(s));
      cjs_ctx_destroy(ctx); ctx = nullptr;
    }
    return cjs_ctx_create_sharded(&ctx, e->device, in_cap, (long)rb, e->level);
  }
  int init() {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return CJS_E_NO_DEVICE;
    if (e->device >= ndev) return CJS_E_INVALID_ARG;
    if (e->device < 0) e->device = 0;
    CJS_HIP_TRY(hipSetDevice(e->device));
    cap = (uint32_t)e->level * 100000u - 19u;
    // the carried block may end inside the new bytes, every further block lies wholly in them and takes >= 4/5 cap of input
    rb = (uint32_t)Rle1Work::max_blocks_for(e->chunk, cap) + 2u;
    in_cap = e->chunk + 2 * (size_t)e->level * 100000 + 4096;
    const size_t per = (size_t)rb * ((size_t)e->level * 100000);
    out_cap = (per + per / 4 + 65536 + 3) & ~(size_t)3;
    for (auto& s : e->slot) CJS_HIP_TRY(hipHostMalloc((void**)s.h.put(), e->chunk));
    CJS_TRY(d_in.alloc(in_cap));
    for (auto& d : d_stage) CJS_TRY(d.alloc(e->chunk));
    for (auto& d : d_out) CJS_TRY(d.alloc(out_cap));
    CJS_HIP_TRY(hipStreamCreateWithFlags(cs.put(), hipStreamNonBlocking));
    for (auto& ev : ev_up) CJS_HIP_TRY(hipEventCreateWithFlags(ev.put(), hipEventDisableTiming));
    CJS_HIP_TRY(hipEventCreateWithFlags(ev_dn.put(), hipEventDisableTiming));
    CJS_HIP_TRY(hipHostMalloc((void**)h_crc.put(), 4 * (size_t)rb));
    CJS_HIP_TRY(hipHostMalloc((void**)h_blk.put(), sizeof(RleBlock)));
    return make_ctx();
  }

  int upload(uint32_t j) {               // staging chunk j -> device staging chunk j, on the copy stream
    Slot& sl = e->slot[j];
    if (sl.n) CJS_HIP_TRY(hipMemcpyAsync(d_stage[j], sl.h, sl.n, hipMemcpyHostToDevice, cs));
    CJS_HIP_TRY(hipEventRecord(ev_up[j], cs));
    sl.uploaded = true;
    return 0;
  }
  // the download in flight has landed: its first byte takes the held-back bits, its last partial byte is held back
  int collect() {
    if (!dl) return 0;
    CJS_HIP_TRY(hipEventSynchronize(ev_dn));
    dl[0] |= hold;
    size_t len = dl_len;
    if (!dl_final && dl_end_phase) { len--; hold = dl[len]; } else hold = 0;
    uint8_t* p = dl;
    dl = nullptr;
    if (!len) { HostPool::give(p); return 0; }
    std::unique_lock<std::mutex> lk(e->mu);
    e->cv.wait(lk, [&] { return !e->pending || e->caller_waits() || e->quit; });
    if (e->quit) { HostPool::give(p); return 0; }
    e->outq.push_back(Piece{p, len, 0});
    e->pending += len;
    return 0;
  }
  // input [from, n) of d_in to its front.  Pieces of at most `from` bytes, in stream order: no copy overlaps itself.
  int move_carry(hipStream_t s, size_t from, size_t n) {
    for (size_t at = from; at < n; at += from)
      CJS_HIP_TRY(hipMemcpyAsync(d_in.p + (at - from), d_in.p + at, std::min(from, n - at), hipMemcpyDeviceToDevice, s));
    return 0;
  }

  int step(uint32_t i) {
    Slot& sl = e->slot[i];
    const size_t n_new = sl.n;
    const bool final = sl.final;
    if (!sl.uploaded) CJS_TRY(upload(i));
    {                                    // the next chunk, when it waits already: its upload runs beside this step's kernels
      std::unique_lock<std::mutex> lk(e->mu);
      Slot& nx = e->slot[i ^ 1];
      const bool go = !final && nx.full && !nx.uploaded;
      lk.unlock();
      if (go) CJS_TRY(upload(i ^ 1));
    }
    const size_t N = carry + n_new;
    if (N > in_cap) {
      CJS_TRY(DevCache::grow(d_in, in_cap, N, true, ctx->stream));
      CJS_TRY(make_ctx());
    }
    hipStream_t s = ctx->stream;
    CJS_HIP_TRY(hipStreamWaitEvent(s, ev_up[i], 0));
    if (n_new) CJS_HIP_TRY(hipMemcpyAsync(d_in.p + carry, d_stage[i], n_new, hipMemcpyDeviceToDevice, s));
    CJS_HIP_TRY(hipEventSynchronize(ev_up[i]));
    {                                    // the staging chunk is free again
      std::lock_guard<std::mutex> lock(e->mu);
      sl.n = 0; sl.full = false; sl.final = false; sl.uploaded = false;
    }
    e->cv.notify_all();
    uint32_t nb = 0, last_len = 0;
    CJS_TRY(rle1_run(s, ctx->rle, d_in, N, &nb, &last_len));
    CJS_TRY(collect());                  // the previous step's bytes came down beside the boundary pass
    if (N && !nb) return CJS_E_HIP;
    const uint32_t cnt = final ? nb : nb - 1;
    size_t out_bytes = 0, next_carry = final ? 0 : N;
    if (cnt) {
      CJS_TRY(blocks_through_tables(ctx, d_in, N, nb, last_len, 0, cnt, nullptr, false));
      if (ctx->side) CJS_HIP_TRY(hipStreamWaitEvent(s, ctx->ev_join, 0));
      CJS_HIP_TRY(hipMemcpyAsync(h_crc, ctx->rle.block_crc, 4 * (size_t)cnt, hipMemcpyDeviceToHost, s));
      if (!final) CJS_HIP_TRY(hipMemcpyAsync(h_blk, ctx->rle.blocks + cnt, sizeof(RleBlock), hipMemcpyDeviceToHost, s));
      const bool index = (e->flags & (CJS_FLAG_ENC_INDEX | CJS_FLAG_ENC_LINES)) != 0;
      if (index) CJS_TRY(enc_rows_enqueue(ctx, d_in, N, 0, cnt, (e->flags & CJS_FLAG_ENC_LINES) != 0));
      CJS_HIP_TRY(hipStreamSynchronize(s));
      if (index) {
        EncRowsWant w;
        enc_rows_collect(ctx, cnt, w);
        bit_at = enc_rows_append(e->ix_entries, e->ix_newlines, w.rows.data(), w.rows.size(), bit_at, e->level);
      }
      for (uint32_t k = 0; k < cnt; k++) scrc = crc_fold(scrc, h_crc[k]);
      if (!final) {
        const uint64_t from = h_blk->s;
        if (from == 0 || from > N) return CJS_E_HIP;
        next_carry = N - (size_t)from;
      }
      const bool header = !header_done;
      const PackShard ps{scrc, 0};
      uint8_t* o = d_out[packs & 1];
      CJS_TRY(pack_enqueue(ctx, PackJob{nb, 0, cnt, header ? 32u : phase, e->level, header, final, ctx->rle.block_crc, ctx->d_pidx, (uint32_t*)o, out_cap, &ps}));
      if (!final) CJS_TRY(move_carry(s, N - next_carry, N));       // (between the two halves: the carry moves beside the wait)
      uint64_t end_bit = 0;
      CJS_TRY(pack_finish(ctx, &end_bit));
      out_bytes = (size_t)((end_bit + 7) / 8);
      // (the packer's end, counted from this step's first byte, against the rows' bits)
      if (index && ((bit_at + (final ? 80 : 0)) & 7) != (end_bit & 7)) return CJS_E_HIP;
      e->ix_end_bit = bit_at;
      dl = (uint8_t*)HostPool::take(out_bytes);
      if (!dl) return CJS_E_OUT_OF_MEMORY;
      dl_len = out_bytes; dl_end_phase = (uint32_t)(end_bit & 7); dl_final = final;
      CJS_HIP_TRY(hipMemcpyAsync(dl, o, out_bytes, hipMemcpyDeviceToHost, cs));
      CJS_HIP_TRY(hipEventRecord(ev_dn, cs));
      header_done = true; phase = dl_end_phase; packs++;
    }
    if (env_debug())
      fprintf(stderr, "[cjs] enc step %u: input %zu B (carry %zu + new %zu), blocks %u of %u packed, %zu B out at bit phase %u, carry %zu B%s\n", steps, N, carry,
              n_new, cnt, nb, out_bytes, phase, next_carry, final ? " (final)" : "");
    carry = next_carry;
    steps++;
    if (final) CJS_TRY(collect());
    return 0;
  }

  int run() {
    int rc = init();
    {
      std::lock_guard<std::mutex> lock(e->mu);
      if (rc) e->fail(rc);
      e->ready = true;
    }
    e->cv.notify_all();
    for (uint32_t i = 0; !rc; i ^= 1) {
      bool final;
      {
        std::unique_lock<std::mutex> lk(e->mu);
        e->cv.wait(lk, [&] { return e->slot[i].full || e->quit; });
        if (e->quit && !e->slot[i].full) break;
        final = e->slot[i].final;
      }
      rc = step(i);
      if (final) break;
    }
    if (!rc) {                           // the stream is complete; the device side stays as it is until the encoder is destroyed
      std::unique_lock<std::mutex> lk(e->mu);
      e->worker_done = true;
      e->cv.notify_all();
      e->cv.wait(lk, [&] { return e->quit; });
    }
    return rc;
  }
};

void worker_main(cjs_bz_enc* e) {
  int rc = 0;
  guarded(rc, [&] { EncWork w(e); rc = w.run(); });
  {
    std::lock_guard<std::mutex> lock(e->mu);
    if (rc) e->fail(rc);
    e->ready = true; e->worker_done = true;
  }
  e->cv.notify_all();
}

// the stream of no input (Q3): header, end-of-stream magic, zero CRC -- nothing for a device to do
int emit_empty(cjs_bz_enc* e) {
  static const uint8_t tail[10] = {0x17, 0x72, 0x45, 0x38, 0x50, 0x90, 0, 0, 0, 0};
  uint8_t* p = (uint8_t*)HostPool::take(14);
  if (!p) return CJS_E_OUT_OF_MEMORY;
  p[0] = 'B'; p[1] = 'Z'; p[2] = 'h'; p[3] = (uint8_t)('0' + e->level);
  memcpy(p + 4, tail, 10);
  e->outq.push_back(Piece{p, 14, 0});
  e->pending += 14;
  return 0;
}

}  // namespace

extern "C" int cjs_bzip2_enc_create(cjs_bz_enc** out, int level, size_t chunk_bytes, const cjs_opts* opts) {
  if (!out) return CJS_E_INVALID_ARG;
  *out = nullptr;
  if (level < 1 || level > 9) return CJS_E_BAD_LEVEL;
  CJS_GUARD_BEGIN
  cjs_bz_enc* e = new cjs_bz_enc();
  e->level = level;
  if (!chunk_bytes) {                    // the default; CJS_ENC_CHUNK_BYTES replaces it (callers without a chunk argument: the JS fronts, cli.js)
    const char* env = getenv("CJS_ENC_CHUNK_BYTES");
    chunk_bytes = env ? (size_t)strtoull(env, nullptr, 10) : 0;
    if (!chunk_bytes) chunk_bytes = ENC_DEFAULT_CHUNK;
  }
  e->chunk = std::min(std::max(chunk_bytes, ENC_MIN_CHUNK), ENC_MAX_CHUNK);
  const Opts o(opts);
  e->device = o.device;
  e->flags = o.flags & (CJS_FLAG_ENC_INDEX | CJS_FLAG_ENC_LINES);
  if (e->device < 0 && hipGetDevice(&e->device) != hipSuccess) { (void)hipGetLastError(); e->device = -1; }      // (no device: the first write says so)
  *out = e;
  return 0;
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

extern "C" int cjs_bzip2_enc_write(cjs_bz_enc* e, const uint8_t* in, size_t n) {
  if (!e) return CJS_E_INVALID_ARG;
  CJS_GUARD_BEGIN
  std::unique_lock<std::mutex> lk(e->mu);
  if (e->rc) return e->rc;
  if ((!in && n) || e->finished) return e->fail(CJS_E_INVALID_ARG);
  if (!n) return 0;
  if (!e->started) {                     // the first byte: the worker makes the device side
    e->worker = std::thread(worker_main, e);
    e->started = true;
    e->cv.wait(lk, [&] { return e->ready; });
  }
  Flag in_write(e->writing);
  while (n) {
    Slot& sl = e->slot[e->wslot];
    if (sl.full) e->cv.notify_all();     // the worker may hold a step's bytes back for a reader: none comes while this waits
    e->cv.wait(lk, [&] { return !sl.full || e->rc; });
    if (e->rc) return e->rc;
    const size_t take = std::min(n, e->chunk - sl.n);
    lk.unlock();
    memcpy(sl.h.p + sl.n, in, take);
    lk.lock();
    sl.n += take; in += take; n -= take;
    if (sl.n == e->chunk) { sl.full = true; e->wslot ^= 1; e->cv.notify_all(); }
  }
  return 0;
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

extern "C" int cjs_bzip2_enc_finish(cjs_bz_enc* e) {
  if (!e) return CJS_E_INVALID_ARG;
  CJS_GUARD_BEGIN
  std::unique_lock<std::mutex> lk(e->mu);
  if (e->rc) return e->rc;
  if (e->finished) return 0;
  e->finished = true;
  if (!e->started) { const int rc = emit_empty(e); return rc ? e->fail(rc) : 0; }
  Flag in_finish(e->finishing);
  e->cv.notify_all();
  Slot& sl = e->slot[e->wslot];
  e->cv.wait(lk, [&] { return !sl.full || e->rc; });
  if (!e->rc) { sl.final = true; sl.full = true; e->cv.notify_all(); }
  e->cv.wait(lk, [&] { return e->worker_done; });
  return e->rc;
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

extern "C" int cjs_bzip2_enc_index(cjs_bz_enc* e, cjs_bz_index** idx, cjs_bz_lines** lines) {
  if (idx) *idx = nullptr;
  if (lines) *lines = nullptr;
  if (!e || !idx) return CJS_E_INVALID_ARG;
  CJS_GUARD_BEGIN
  std::lock_guard<std::mutex> lock(e->mu);
  if (e->rc) return e->rc;
  if (!e->flags || (lines && !(e->flags & CJS_FLAG_ENC_LINES))) return CJS_E_INVALID_ARG;
  if (!e->finished || (e->started && !e->worker_done)) return CJS_E_INVALID_ARG;      // finish() has not returned 0
  return enc_tables_make(e->ix_entries, e->ix_newlines, e->ix_end_bit, idx, lines);
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

extern "C" size_t cjs_bzip2_enc_pending(const cjs_bz_enc* ce) {
  if (!ce) return 0;
  cjs_bz_enc* e = const_cast<cjs_bz_enc*>(ce);
  std::lock_guard<std::mutex> lock(e->mu);
  return e->rc ? 0 : e->pending;
}

extern "C" int cjs_bzip2_enc_read(cjs_bz_enc* e, uint8_t* out, size_t cap, size_t* got) {
  if (got) *got = 0;
  if (!e) return CJS_E_INVALID_ARG;
  std::lock_guard<std::mutex> lock(e->mu);
  if (e->rc) return e->rc;
  if (!got || (!out && cap)) return e->fail(CJS_E_INVALID_ARG);
  size_t done = 0;
  while (done < cap && !e->outq.empty()) {
    Piece& p = e->outq.front();
    const size_t take = std::min(cap - done, p.len - p.off);
    memcpy(out + done, p.p + p.off, take);
    p.off += take; done += take;
    if (p.off == p.len) { HostPool::give(p.p); e->outq.pop_front(); }
  }
  e->pending -= done;
  *got = done;
  if (done && !e->pending) e->cv.notify_all();      // the worker may wait with the next step's bytes
  return 0;
}

extern "C" void cjs_bzip2_enc_destroy(cjs_bz_enc* e) {
  if (!e) return;
  {
    std::lock_guard<std::mutex> lock(e->mu);
    e->quit = true;
  }
  e->cv.notify_all();
  if (e->worker.joinable()) e->worker.join();
  for (auto& p : e->outq) HostPool::give(p.p);
  delete e;
}
