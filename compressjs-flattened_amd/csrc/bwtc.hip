// bwtc.hip — BWTC.compressFile (J/BWTC_joined_.js:1698-1825) and BWTC.decompressFile (:1827-1920) on the MI355X: the host drivers.
//
// Per block (level*100000 input bytes, no RLE1): sentinel BWT (bwt.hip, shared with bzip2) -> symbol map +
// MTF + RLE2 (mtf.hip, shared: the RLE2 stream is bzip2's minus the EOB symbol, J/BWTC_joined_.js:1767-1819)
// -> adaptive model evaluation on the GPU (bwtc_model.hip), which leaves each block's list of coder steps (bwtc_format.h).
// The range coder itself (RangeCoder :40-153) carries ONE (low, range) state across all blocks (:1699):
// range' = floor(range / tot) * sy is a serial integer chain over the whole file, so that tail runs on
// one host thread, in block order, over the GPU-produced steps: HostCoder and the framing of bwtc_host.h.
// Decompression is the serial entropy stage of bwtc_decode.h on the host and the inverse BWT of all blocks on the GPU.
#include "cjs_internal.h"
#include "host.h"
#include "mtf.h"
#include "bwtc_host.h"
#include "bwtc_decode.h"
#include <stdlib.h>
#include <string.h>
#include <sched.h>
#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <vector>

using namespace cjs;

// One batch of consecutive blocks: BWT -> MTF/RLE2 -> model evaluation on one GPU (worker thread), leaving the per-block
// step lists in HBM until the coder has consumed them.  The batches are those of plan_batches (bwtc_host.h); at most two
// batches per slot are alive.
namespace {

using Clock = std::chrono::steady_clock;
double ms_since(Clock::time_point a) { return std::chrono::duration<double, std::milli>(Clock::now() - a).count(); }

struct BwtcBatch : BatchPlan {
  int rc = 0;
  bool done = false;
  struct Gpu {                                 // destroyed in reverse order: events, streams, then the workspace
    Arena arena; BwtWork bw;
    Stream s, cs;                             // work stream, copy stream (step lists -> pinned host buffers)
    Event cev[2];
  };
  std::unique_ptr<Gpu> g;
  uint64_t* d_steps = nullptr; size_t step_stride = 0;
  std::vector<uint32_t> pidx, asz, nsteps; std::vector<uint8_t> alist;
  double ms = 0;
  void release() {                            // once its streams have drained, on its device
    if (!g || hipSetDevice(device) != hipSuccess) return;
    if (g->s) (void)hipStreamSynchronize(g->s);
    if (g->cs) (void)hipStreamSynchronize(g->cs);
    g.reset();
  }
};

struct BwtcJob {
  const uint8_t* in = nullptr; size_t n = 0;
  uint32_t bs = 0, nb = 0, n_last = 0; bool fast = false;
  std::vector<BwtcBatch> batches;
  std::mutex mu; std::condition_variable cv;
  std::vector<int> live, next_seq;            // per slot: batches alive, next batch allowed to start
  bool abort = false;
};

// a batch's device rows beside the MTF workspace, all carved from its arena
struct BatchRows {
  MtfWork mw;
  uint8_t *d_T = nullptr, *d_U = nullptr;
  uint32_t *d_pidx = nullptr, *d_len = nullptr, *d_nsteps = nullptr;
};

// waits for the batch's turn (its slot's batches start in order, at most two alive); false: the job was stopped
bool batch_admit(BwtcJob* J, BwtcBatch* B) {
  std::unique_lock<std::mutex> lk(J->mu);
  J->cv.wait(lk, [&] { return J->abort || (J->next_seq[B->slot] == B->seq && J->live[B->slot] < 2); });
  if (J->abort) { B->rc = CJS_E_HIP; B->done = true; J->next_seq[B->slot]++; J->cv.notify_all(); return false; }
  J->live[B->slot]++; J->next_seq[B->slot]++;
  J->cv.notify_all();
  return true;
}
int batch_carve(const BwtcJob& J, BwtcBatch& B, BatchRows& R) {
  const uint32_t bs = J.bs, cnt = B.count;
  const size_t elems = (size_t)cnt * bs;
  BwtcBatch::Gpu& G = *B.g;
  CJS_TRY(G.arena.init_pooled(BwtWork::bytes_needed(elems) + MtfWork::bytes_needed(cnt, bs) + 2 * (elems + 512) + 8 * (size_t)cnt * B.step_stride + 16 * (size_t)cnt + 65536));
  CJS_TRY(G.bw.carve(G.arena, elems));
  CJS_TRY(R.mw.carve(G.arena, cnt, bs));
  R.d_T = G.arena.take<uint8_t>(elems); R.d_U = G.arena.take<uint8_t>(elems);
  R.d_pidx = G.arena.take<uint32_t>(cnt); R.d_len = G.arena.take<uint32_t>(cnt); R.d_nsteps = G.arena.take<uint32_t>(cnt);
  B.d_steps = G.arena.take<uint64_t>((size_t)cnt * B.step_stride);
  return B.d_steps ? 0 : (int)CJS_E_OUT_OF_MEMORY;
}
int batch_streams(const BwtcJob& J, BwtcBatch& B) {
  BwtcBatch::Gpu& G = *B.g;
  if (B.slot == 0 && B.seq == 0 && J.batches.size() > 1) {   // the batch the coder is waiting for goes ahead of the others' kernels
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess) (void)hipStreamCreateWithPriority(G.s.put(), hipStreamDefault, greatest);
  }
  if ((!G.s && hipStreamCreate(G.s.put()) != hipSuccess) || hipStreamCreate(G.cs.put()) != hipSuccess ||
      hipEventCreateWithFlags(G.cev[0].put(), hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(G.cev[1].put(), hipEventDisableTiming) != hipSuccess) return CJS_E_HIP;
  return 0;
}
// input up, BWT -> MTF/RLE2 -> model, the per-block facts of the block heads down; the step lists stay on the device
int batch_run(const BwtcJob& J, BwtcBatch& B, BatchRows& R) {
  const uint32_t bs = J.bs, cnt = B.count;
  const uint32_t n_last = B.first + cnt == J.nb ? J.n_last : bs;
  const size_t nbytes = (size_t)(cnt - 1) * bs + n_last;
  std::vector<uint32_t> lens(cnt, bs); lens[cnt - 1] = n_last;
  hipStream_t s = B.g->s;
  if (hipMemcpyAsync(R.d_T, J.in + (size_t)B.first * bs, nbytes, hipMemcpyHostToDevice, s) != hipSuccess) return CJS_E_HIP;
  if (hipMemcpyAsync(R.d_len, lens.data(), 4 * (size_t)cnt, hipMemcpyHostToDevice, s) != hipSuccess) return CJS_E_HIP;
  CJS_TRY(bwt_run(s, B.g->bw, R.d_T, cnt, bs, n_last, false, R.d_U, R.d_pidx, nullptr));
  CJS_TRY(mtf_run(s, R.mw, R.d_U, cnt, R.d_len));
  CJS_TRY(bwtc_model_launch(s, J.fast, R.mw.b, cnt, B.d_steps, B.step_stride, R.d_nsteps));
  if (hipMemcpyAsync(B.pidx.data(), R.d_pidx, 4 * (size_t)cnt, hipMemcpyDeviceToHost, s) != hipSuccess) return CJS_E_HIP;
  if (hipMemcpyAsync(B.asz.data(), R.mw.b.asz, 4 * (size_t)cnt, hipMemcpyDeviceToHost, s) != hipSuccess) return CJS_E_HIP;
  if (hipMemcpyAsync(B.nsteps.data(), R.d_nsteps, 4 * (size_t)cnt, hipMemcpyDeviceToHost, s) != hipSuccess) return CJS_E_HIP;
  if (hipMemcpyAsync(B.alist.data(), R.mw.b.alist, (size_t)cnt * 256, hipMemcpyDeviceToHost, s) != hipSuccess) return CJS_E_HIP;
  return hipStreamSynchronize(s) != hipSuccess ? (int)CJS_E_HIP : 0;      // (lens is read by the copy until here)
}
void bwtc_batch_body(BwtcJob* J, BwtcBatch* B) {
  if (!batch_admit(J, B)) return;
  const auto T0 = Clock::now();
  const uint32_t cnt = B->count;
  int rc = hipSetDevice(B->device) != hipSuccess ? (int)CJS_E_HIP : 0;
  B->g.reset(new BwtcBatch::Gpu());
  B->step_stride = 2 * MtfWork::a_stride_for(J->bs);
  B->pidx.resize(cnt); B->asz.resize(cnt); B->nsteps.resize(cnt); B->alist.resize((size_t)cnt * 256);
  BatchRows R;
  if (!rc) rc = batch_carve(*J, *B, R);
  if (!rc) rc = batch_streams(*J, *B);
  if (!rc) rc = batch_run(*J, *B, R);
  B->ms = ms_since(T0);
  std::lock_guard<std::mutex> lk(J->mu);
  B->rc = rc; B->done = true;
  if (rc) J->abort = true;
  J->cv.notify_all();
}
// an exception of the body becomes the batch's return code and stops the job
void bwtc_batch_worker(BwtcJob* J, BwtcBatch* B) {
  int rc = 0;
  guarded(rc, [&] { bwtc_batch_body(J, B); });
  if (!rc) return;
  std::lock_guard<std::mutex> lk(J->mu);
  B->rc = rc; B->done = true; J->abort = true;
  J->cv.notify_all();
}

// The workers of a job, stopped and joined on every path out of the scope that started them; the batches then give their
// device memory back.
struct Stop {
  BwtcJob& J; Workers th;
  ~Stop() {
    if (!th.th.empty()) { { std::lock_guard<std::mutex> lk(J.mu); J.abort = true; } J.cv.notify_all(); th.join(); }
    for (auto& B : J.batches) B.release();
  }
};

// The step lists on their way to the coder: the steps of block k+1 travel (pinned buffer k+1 & 1, copy stream of its batch)
// while block k goes through the coder.
struct StepFeed {
  BwtcJob& J;
  Pinned<uint64_t> h_buf[2];
  hipEvent_t pending[2] = {nullptr, nullptr}; int pending_dev[2] = {0, 0};
  size_t bi_of_next = 0;                                           // batch that holds the next block to fetch
  double ms_stall = 0;                                             // the coder waited for the GPU
  int init(size_t step_stride) {
    if (hipHostMalloc((void**)h_buf[0].put(), 8 * step_stride, hipHostMallocPortable) != hipSuccess || hipHostMalloc((void**)h_buf[1].put(), 8 * step_stride, hipHostMallocPortable) != hipSuccess) return CJS_E_HIP;
    return 0;
  }
  int batch_done(size_t bi) {                                      // blocks until the batch's GPU work is done
    const auto Tw = Clock::now();
    std::unique_lock<std::mutex> lk(J.mu);
    J.cv.wait(lk, [&] { return J.batches[bi].done; });
    ms_stall += ms_since(Tw);
    return J.batches[bi].rc;
  }
  int fetch(uint32_t k) {                                          // starts the copy of block k's steps
    while (J.batches[bi_of_next].first + J.batches[bi_of_next].count <= k) bi_of_next++;
    BwtcBatch& B = J.batches[bi_of_next];
    CJS_TRY(batch_done(bi_of_next));
    const uint32_t r = k - B.first;
    if (hipSetDevice(B.device) != hipSuccess) return (int)CJS_E_HIP;
    if (B.nsteps[r] && hipMemcpyAsync(h_buf[k & 1], B.d_steps + (size_t)r * B.step_stride, 8 * (size_t)B.nsteps[r], hipMemcpyDeviceToHost, B.g->cs) != hipSuccess) return (int)CJS_E_HIP;
    if (hipEventRecord(B.g->cev[k & 1], B.g->cs) != hipSuccess) return (int)CJS_E_HIP;
    pending[k & 1] = B.g->cev[k & 1]; pending_dev[k & 1] = B.device;
    return 0;
  }
  const uint64_t* wait(uint32_t k) {                               // block k's steps once they have arrived; null: a HIP call failed
    if (hipSetDevice(pending_dev[k & 1]) != hipSuccess || hipEventSynchronize(pending[k & 1]) != hipSuccess) return nullptr;
    return h_buf[k & 1];
  }
  void retire(size_t bi) {                                         // the coder is through with the batch: give its memory back
    BwtcBatch& B = J.batches[bi];
    B.release();
    std::lock_guard<std::mutex> lk(J.mu);
    J.live[B.slot]--;
    J.cv.notify_all();
  }
};

// every block through the coder, in order: its head, then its step list
int code_block_loop(BwtcJob& J, StepFeed& feed, HostCoder& coder, double& ms_coder) {
  const uint64_t* rc_tab = rcp_table();
  size_t bi_cur = 0;
  for (uint32_t k = 0; k < J.nb; k++) {
    while (J.batches[bi_cur].first + J.batches[bi_cur].count <= k) { feed.retire(bi_cur); bi_cur++; }
    const BwtcBatch& B = J.batches[bi_cur];
    const uint32_t r = k - B.first;
    if (k + 1 < J.nb) CJS_TRY(feed.fetch(k + 1));
    const auto Tc = Clock::now();
    coder.reserve_steps(B.nsteps[r]);                              // everything this block can emit
    code_block_head(coder, J.bs, k + 1 == J.nb ? J.n_last : J.bs, B.pidx[r], B.alist.data() + (size_t)r * 256, B.asz[r]);
    const uint64_t* steps = feed.wait(k);
    if (!steps) return CJS_E_HIP;
    code_steps(coder, steps, B.nsteps[r], rc_tab);
    ms_coder += ms_since(Tc);
  }
  return 0;
}

void report_blocks(const BwtcJob& J, const Opts& op, int rc, Clock::time_point T0, double ms_first, double ms_gpu_max, double ms_coder, double ms_stall) {
  if (env_debug()) fprintf(stderr, "[cjs bwtc] %zu batch(es) on %u slot(s): first step list after %.1f ms, longest batch (workspace + H2D + BWT + MTF + model) %.1f ms, "
                                   "range coder over the step lists (host, serial) %.1f ms, coder waited for the GPU %.1f ms, total %.1f ms\n",
                           J.batches.size(), (unsigned)J.live.size(), ms_first, ms_gpu_max, ms_coder, ms_stall, ms_since(T0));
  cjs_stats* st = op.stats;
  if (st && !rc) {                                                 // BWTC meaning of the fields: see include/cjs_hip.h
    memset(st, 0, sizeof *st);
    st->ms_total = ms_since(T0); st->ms_bwt = ms_gpu_max; st->ms_pack = ms_coder; st->ms_rle1 = ms_stall; st->ms_mtf = ms_first;
    st->blocks = J.nb; st->bytes_in = J.n;
  }
}

// The blocks of a job (J.nb > 0): plan the batches, start their workers, run the coder over the step lists as they arrive.
int code_blocks(BwtcJob& J, HostCoder& coder, const Opts& op, int ndev, int dev0) {
  const auto T0 = Clock::now();
  static const uint32_t first_batch = getenv("CJS_BWTC_FIRST_BATCH") ? (uint32_t)atoi(getenv("CJS_BWTC_FIRST_BATCH")) : BWTC_FIRST_BATCH;
  const uint32_t nslots = plan_slots(op.n_devices, J.nb);
  J.live.assign(nslots, 0); J.next_seq.assign(nslots, 0);
  const std::vector<BatchPlan> plan = plan_batches(J.nb, nslots, ndev, dev0, first_batch);
  J.batches.resize(plan.size());
  for (size_t i = 0; i < plan.size(); i++) static_cast<BatchPlan&>(J.batches[i]) = plan[i];
  // on every path out of this scope (an exception of the coder side included: out.resize in reserve_steps) the workers are
  // stopped and joined, the batches give their device memory back, device dev0 is made current again and the pinned step
  // buffers are freed (members and locals go in reverse order)
  StepFeed feed{J};
  RestoreDevice restore{dev0};
  Stop wk{J};
  for (auto& B : J.batches) wk.th.run(B.rc, [&J, &B] { bwtc_batch_worker(&J, &B); });     // (the worker's own guard leaves the outer one nothing to catch)
  int rc = feed.init(2 * MtfWork::a_stride_for(J.bs));
  if (!rc) rc = feed.fetch(0);
  const double ms_first = ms_since(T0);
  double ms_coder = 0;
  if (!rc) rc = code_block_loop(J, feed, coder, ms_coder);
  if (rc) { std::lock_guard<std::mutex> lk(J.mu); J.abort = true; J.cv.notify_all(); }
  wk.th.join();
  double ms_gpu_max = 0;
  for (auto& B : J.batches) { if (!rc && B.rc) rc = B.rc; ms_gpu_max = std::max(ms_gpu_max, B.ms); }
  report_blocks(J, op, rc, T0, ms_first, ms_gpu_max, ms_coder, feed.ms_stall);
  return rc;
}

}  // namespace

extern "C" int cjs_bwtc_compress(const uint8_t* in, size_t n, int level, uint8_t** out, size_t* out_n, const cjs_opts* opts) {
  if (!out || !out_n) return CJS_E_INVALID_ARG;
  *out = nullptr; *out_n = 0;
  clear_detail();
  CJS_GUARD_BEGIN
  CJS_TRY(select_device(opts));
  if (level < 1 || level > 9) level = 9;                             // J/BWTC_joined_.js:1702-1705
  int ndev = 0, dev0 = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || hipGetDevice(&dev0) != hipSuccess) return CJS_E_NO_DEVICE;
  BwtcJob J;
  J.in = in; J.n = n; J.fast = level <= 5; J.bs = (uint32_t)level * 100000u;
  J.nb = (uint32_t)((n + J.bs - 1) / J.bs);
  J.n_last = J.nb ? (uint32_t)(n - (size_t)(J.nb - 1) * J.bs) : 0;
  const Opts op(opts);
  std::vector<uint8_t> o;
  o.reserve(n / 3 + 64);
  const int first_byte = write_stream_head(o, n, (op.flags & CJS_FLAG_SIZE_UNKNOWN) != 0);
  HostCoder coder(o);
  coder.start(first_byte, 1);                                        // :1700 (the last varint byte is the coder's first byte)
  static const bool env_split_coder = getenv("CJS_BWTC_SPLIT_CODER") == nullptr || atoi(getenv("CJS_BWTC_SPLIT_CODER")) != 0;
  const int dbg_cpu0 = sched_getcpu();
  if (env_split_coder && J.nb) coder.start_split();                  // range chain here, low chain on a second host thread
  coder.shift(1, (uint32_t)level, 8);                                // encodeByte(level) :1706
  if (J.nb) CJS_TRY(code_blocks(J, coder, op, ndev, dev0));
  coder.reserve_steps(64);
  coder.freq(1, 2, 3);                                               // "no more blocks" :1823
  const int dbg_cpu1 = sched_getcpu();
  coder.finish();
  if (coder.failed.load()) return CJS_E_OUT_OF_MEMORY;
  if (env_debug()) fprintf(stderr, "[cjs bwtc] split coder: range side on cpu %d -> %d, low side on cpu %d -> %d, polls with the ring full %llu, empty %llu\n", dbg_cpu0, dbg_cpu1,
                           coder.dbg_low_cpu[0], coder.dbg_low_cpu[1], (unsigned long long)coder.dbg_full_spins, (unsigned long long)coder.dbg_empty_spins);
  CJS_TRY(malloc_result(o, out, out_n));
  if (op.stats) op.stats->bytes_out = o.size();
  return 0;
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

// ---------------------------------------------------------------- stage-level entry points (tests; host only, no device is touched)
// The host range coder on a caller-made step list: encodeStart(first_byte, 1), the compressor's step loop, encodeFinish.
// mode 0 = both chains on the calling thread, 1 = split across two threads.
extern "C" int cjs_stage_bwtc_code(const uint64_t* steps, size_t n, int first_byte, int mode, uint8_t** out, size_t* out_n) {
  if (!out || !out_n) return CJS_E_INVALID_ARG;
  *out = nullptr; *out_n = 0;
  CJS_GUARD_BEGIN
  if ((n && !steps) || n > (1u << 30) || first_byte < 0 || first_byte > 255 || (mode != 0 && mode != 1)) return CJS_E_INVALID_ARG;
  for (size_t i = 0; i < n; i++) if (!step_valid(steps[i])) return CJS_E_INVALID_ARG;      // a step the reference's models could not make is refused, not coded
  std::vector<uint8_t> o;
  HostCoder coder(o);
  coder.start(first_byte, 1);
  if (mode == 1) coder.start_split();
  coder.reserve_steps(n);
  code_steps(coder, steps, (uint32_t)n, rcp_table());
  coder.reserve_steps(64);
  coder.finish();
  if (coder.failed.load()) return CJS_E_OUT_OF_MEMORY;
  return malloc_result(o, out, out_n);
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

// The serial entropy stage of BWTC.decompressFile (bwtc_decode.h).
// cols receives the BWT columns of all non-empty blocks back to back (malloc'd, cjs_free); lens/pidx per block.
extern "C" long cjs_stage_bwtc_entropy_decode(const uint8_t* in, size_t n, uint8_t** cols, size_t* cols_n, uint32_t* lens, uint32_t* pidx, long cap,
                                              int* level) {
  if (!cols || !cols_n) return CJS_E_INVALID_ARG;
  *cols = nullptr; *cols_n = 0;
  CJS_GUARD_BEGIN
  BwtcBlocks B;
  const int rc = bwtc_entropy_decode(in, n, B, env_debug());
  if (rc) return (long)rc;
  if (level) *level = B.level;
  if (malloc_result(B.cols, cols, cols_n)) return (long)CJS_E_OUT_OF_MEMORY;
  for (size_t k = 0; k < B.lens.size() && (long)k < cap; k++) { if (lens) lens[k] = B.lens[k]; if (pidx) pidx[k] = B.pidx[k]; }
  return (long)B.lens.size();
  CJS_GUARD_END((long)CJS_E_OUT_OF_MEMORY, (long)CJS_E_HIP)
}

// ---------------------------------------------------------------- BWTC.decompressFile (J/BWTC_joined_.js:1827-1920)
extern "C" int cjs_bwtc_decompress(const uint8_t* in, size_t n, uint8_t** out, size_t* out_n, const cjs_opts* opts) {
  if (!out || !out_n) return CJS_E_INVALID_ARG;
  *out = nullptr; *out_n = 0;
  clear_detail();
  CJS_GUARD_BEGIN
  CJS_TRY(select_device(opts));
  BwtcBlocks B;
  CJS_TRY(bwtc_entropy_decode(in, n, B, env_debug()));
  const uint32_t nb = (uint32_t)B.lens.size();
  const uint64_t total = B.cols.size();
  std::unique_ptr<uint8_t, void (*)(void*)> host((uint8_t*)malloc(total ? (size_t)total : 1), free);
  if (!host) return CJS_E_OUT_OF_MEMORY;
  if (nb) {
    // n <= 1 blocks: unbwtransform copies (:1149-1152); handled by the same kernels (a 1-element chain)
    DevMem<uint8_t> d_T, d_out;
    Stream s;
    CJS_TRY(d_T.alloc((size_t)total + 64));
    CJS_TRY(d_out.alloc((size_t)total + 64));
    CJS_HIP_TRY(hipStreamCreate(s.put()));
    CJS_HIP_TRY(hipMemcpyAsync(d_T, B.cols.data(), (size_t)total, hipMemcpyHostToDevice, s));
    CJS_TRY(ibwt_sentinel_run(s, d_T, (uint32_t)B.level * 100000u, nb, B.lens.data(), B.pidx.data(), d_out));
    if (total) CJS_HIP_TRY(hipMemcpy(host.get(), d_out, (size_t)total, hipMemcpyDeviceToHost));
  }
  *out = host.release(); *out_n = (size_t)total;
  return 0;
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}
