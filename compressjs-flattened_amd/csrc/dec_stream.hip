// dec_stream.hip -- the streaming Bzip2 decoder (cjs_bzip2_dec_*, Bzip2Decoder, Bzip2.decompressStream): the counterpart of
// enc_stream.hip.  The phases of the decode engine (dec_engine.h, decode.hip) over a sliding window of the stream.  The decoder keeps
// the stream bytes from the carry point on (host copy;
// uploaded per step at their absolute byte offset, so the dword phase holds), the walk state (WalkState: bit position, folded
// stream CRC, the member's block size) and one output buffer of out_bytes.  A step: phase A over the window with rows for the
// first R block candidates at the walk position; bz_walk resumed from the kept state, stopping in front of whatever the bytes
// still to come could change; phase B over the chain; the chain cut to the output budget (the walk state rolled back to the first
// block not emitted); phase C into the device output buffer and one D2H.  All device scratch comes from the decoder's DecArena.
// Synchronous: no worker thread.  See DESIGN.md §6f.
#include "dec_engine.h"
#include <stdlib.h>
#include <string.h>

using namespace cjs;

namespace {
constexpr size_t DEC_DEFAULT_CHUNK = (size_t)64 << 20, DEC_DEFAULT_OUT = (size_t)256 << 20;      // DESIGN.md §6f (placeholders, UNMEASURED)
constexpr size_t DEC_MIN_CHUNK = (size_t)64 << 10, DEC_MAX_CHUNK = (size_t)1 << 30;
const char* const WALK_WHY[] = {"runs", "end of stream", "block magic not all here", "stream crc not all here", "member header not all here", "candidate without a row",
                                "block not all here", "error too near the end", "output budget"};
struct WinBytes {                        // the window by absolute stream byte
  const uint8_t* p; uint64_t off;
  uint8_t operator[](uint64_t i) const { return p[i - off]; }
};
}  // namespace

struct cjs_bz_dec {
  int multistream = 0, device = -1;
  size_t chunk = 0, out_req = 0;
  bool eager = false, debug = false;
  int rc = 0; char detail[192] = {0};      // first failure: every later call returns it
  // input window: stream bytes [win_off, win_off + win_len); the first `seen` of them have been through a step
  uint8_t* win = nullptr; size_t win_cap = 0, win_len = 0, seen = 0; uint64_t win_off = 0, written = 0;
  bool win_pinned = false, finished = false, header_ok = false, ended = false, dev_ready = false;
  int level = 0;                           // of the header; rows and blocks are sized for L = 9 with multistream
  uint32_t tt_stride = 0, rows = 0;
  WalkState W;
  // output of the last step: held - held_pos bytes still to be read; then the pending verdict
  size_t out_cap = 0, held = 0, held_pos = 0;
  Pinned<uint8_t> h_out; DevMem<uint8_t> d_out;
  int pend_rc = 0; char pend_detail[192] = {0};
  DecArena arena; Stream s;
  uint32_t steps = 0;
  int fail(int code, const char* text) {
    if (!rc) { rc = code; snprintf(detail, sizeof detail, "%s", text ? text : ""); }
    clear_detail();
    if (detail[0]) set_detail("%s", detail);
    return rc;
  }
  ~cjs_bz_dec() {
    int cur = 0;
    if (dev_ready && hipGetDevice(&cur) == hipSuccess) {
      RestoreDevice restore{cur};          // the caller's device stays current
      if (hipSetDevice(device) == hipSuccess) {
        if (s) (void)hipStreamSynchronize(s);
        if (win_pinned) (void)hipHostUnregister(win);
        s.reset(); h_out.reset(); d_out.reset(); arena.release();
      }
    }
    free(win);
  }
};

namespace {

// _start_bunzip (:1408-1427) on the first four bytes: no device
int dec_header(cjs_bz_dec* d) {
  const char* why = nullptr;
  if (bz_header_check(d->win, d->written, &d->level, &why)) return d->fail(CJS_E_NOT_BZIP_DATA, why);
  const uint32_t L = d->multistream ? 9u : (uint32_t)d->level;      // later members cannot be seen ahead
  d->tt_stride = 100000u * L;
  d->out_cap = std::max<size_t>(d->out_req ? d->out_req : DEC_DEFAULT_OUT, (size_t)52 * d->tt_stride);
  d->rows = (uint32_t)std::min<size_t>(65535, std::max<size_t>(1, d->out_cap / d->tt_stride));
  d->W = WalkState{};
  d->W.dbuf_size = 100000u * (uint32_t)d->level;
  d->header_ok = true;
  return 0;
}

int dec_device_init(cjs_bz_dec* d) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return CJS_E_NO_DEVICE; }
  if (d->device >= ndev) return CJS_E_INVALID_ARG;
  if (d->device < 0 && hipGetDevice(&d->device) != hipSuccess) return CJS_E_NO_DEVICE;
  CJS_HIP_TRY(hipSetDevice(d->device));
  d->dev_ready = true;
  CJS_HIP_TRY(hipStreamCreate(d->s.put()));
  if (hipHostRegister(d->win, d->win_cap, hipHostRegisterDefault) == hipSuccess) d->win_pinned = true; else (void)hipGetLastError();
  CJS_HIP_TRY(hipHostMalloc((void**)d->h_out.put(), d->out_cap));
  CJS_TRY(d->d_out.alloc(d->out_cap + 256));
  // rows ~10 B and inverse BWT ~24 B per byte of rows x block size, the window twice (upload + candidates)
  return d->arena.init((size_t)28 * d->rows * ((size_t)d->tt_stride + 4096) + 2 * d->win_cap + ((size_t)16 << 20));
}

int dec_step(cjs_bz_dec* d) {
  int cur = 0;
  if (!d->dev_ready) {
    const bool had = hipGetDevice(&cur) == hipSuccess;
    const int rc = dec_device_init(d);
    if (rc) { if (had) (void)hipSetDevice(cur); return rc; }
    if (had) (void)hipSetDevice(cur);
  }
  if (hipGetDevice(&cur) != hipSuccess) return CJS_E_NO_DEVICE;
  RestoreDevice restore{cur};
  CJS_HIP_TRY(hipSetDevice(d->device));
  const bool final = d->finished, was_full = d->win_len == d->win_cap;
  const uint32_t spills0 = d->arena.spills;
  const uint64_t n = d->win_off + d->win_len, pos0 = d->W.pos;
  const size_t len0 = d->win_len;
  DecJob J; J.n = (size_t)n; J.mode = 0; J.timing = env_debug(); J.tt_stride = d->tt_stride; J.batch = true;
  DecShare S; S.device = d->device; S.arena = &d->arena; S.s = std::move(d->s);
  struct Back { cjs_bz_dec* d; DecShare& S; ~Back() { S.release_keep_stream(d->s); } } back{d, S};      // on every path out
  S.lo = S.up_lo = d->win_off; S.hi = S.up_hi = n; S.row_limit = d->rows; S.row_from = d->W.pos;
  J.upload = [d](DecShare* sh, uint8_t* dst) {
    if (d->win_len && hipMemcpyAsync(dst, d->win, d->win_len, hipMemcpyHostToDevice, sh->s) != hipSuccess) return (int)CJS_E_HIP;
    sh->h2d += d->win_len;
    return 0;
  };
  guarded(S.rc, [&] { dec_phase_a(&J, &S); });
  if (S.rc) return S.rc;
  // ---- the walk, resumed
  WalkState& W = d->W;
  W.partial = !final; W.cut_bit = S.cut_bit; W.extent = dec_extent(d->tt_stride); W.stop = WALK_RUNS;
  std::vector<WalkState> before;           // the state in front of each chain block
  clear_detail();
  int wrc = walk_chain(J, WalkCands(&S, 1), WinBytes{d->win, d->win_off}, (size_t)n, d->multistream, 0,
                       [&](long ci, uint64_t) { if (S.cands[(size_t)ci].kind == 0) before.push_back(W); }, &W);
  char wdetail[192];
  snprintf(wdetail, sizeof wdetail, "%s", cjs_last_error_detail());
  clear_detail();
  // ---- phase B over the chain, then the cut to the output budget
  size_t nb = J.chain.size();
  const size_t walked = nb;
  if (nb) {
    S.c0 = 0; S.c1 = nb;
    guarded(S.rc, [&] { dec_phase_b(&J, &S); });
    if (S.rc) return S.rc;
  }
  chain_out_offsets(J);
  if (nb) {
    if (J.out_off[1] > d->out_cap) return CJS_E_UNSUPPORTED;      // cannot happen: out_cap >= a block's largest expansion
    size_t k = 1;
    while (k < nb && J.out_off[k + 1] <= d->out_cap) k++;
    if (k < nb) {                          // block k and what the walk met behind it: the next step's
      const WalkState& b = before[k];
      W.pos = b.pos; W.crc = b.crc; W.dbuf_size = b.dbuf_size; W.stop = WALK_OUT_BUDGET;
      wrc = 0;
      J.chain.resize(k); J.out_off.resize(k + 1); S.c1 = nb = k;
    }
    // ---- phase C: a CRC verdict per block; the first bad block in chain order comes before the walk's error
    J.dev_out = d->d_out; J.host = nullptr; J.crc_got.assign(nb, 0);
    S.rc = 0;
    guarded(S.rc, [&] { dec_phase_c(&J, &S); });
    if (S.rc) return S.rc;
  }
  size_t bad = 0;
  while (bad < nb && J.crc_got[bad] == J.chain[bad].crc) bad++;
  const size_t deliver = (size_t)J.out_off[bad];
  if (deliver) { CJS_HIP_TRY(hipMemcpyAsync(d->h_out, d->d_out, deliver, hipMemcpyDeviceToHost, S.s)); CJS_HIP_TRY(hipStreamSynchronize(S.s)); S.d2h += deliver; }
  d->held = deliver; d->held_pos = 0;
  if (bad < nb) {                          // Bad block CRC (:1756-1761): nothing of the block is delivered
    d->pend_rc = CJS_E_DATA_ERROR;
    bad_crc_detail(d->pend_detail, sizeof d->pend_detail, J.crc_got[bad], J.chain[bad].crc);
  } else if (wrc) {
    d->pend_rc = wrc;
    snprintf(d->pend_detail, sizeof d->pend_detail, "%s", wdetail);
  } else if (W.stop == WALK_ENDED) d->ended = true;
  // ---- the carry: the window from the walk position's byte on
  if (!d->pend_rc) {
    const uint64_t keep_from = d->ended ? n : std::min<uint64_t>(W.pos >> 3, n);
    const size_t gone = (size_t)(keep_from - d->win_off);
    if (gone) memmove(d->win, d->win + gone, d->win_len - gone);
    d->win_off = keep_from; d->win_len -= gone;
  }
  d->seen = d->win_len;
  if (d->debug)
    fprintf(stderr, "[cjs dec step] %u: window %zu B at byte %llu, carry %zu B, candidates %u rows %u, blocks walked %zu emitted %zu, %zu B out, walk stopped: %s%s%s\n",
            d->steps, len0, (unsigned long long)(n - len0), d->win_len, S.ncand_seen, S.nrows_given(), walked, std::min(bad, nb), deliver,
            d->pend_rc ? "error" : WALK_WHY[W.stop], final ? " (final)" : "", d->arena.spills != spills0 ? " [arena spilled]" : "");
  d->steps++;
  // (cannot happen: a full window holds a whole block behind the walk position, and the final steps end or emit)
  if (!d->pend_rc && !d->ended && (final ? W.pos == pos0 : was_full && d->win_len == d->win_cap)) return CJS_E_UNSUPPORTED;
  return 0;
}

// A full window always has fresh bytes: the step that last ran on a full window either moved the walk position, and with it the
// carry point (a block, an end-of-stream record or a member header: whole bytes each), so the window was no longer full and only
// a _write can have filled it again; or it failed the decoder (CJS_E_UNSUPPORTED in dec_step).  So a _write that took nothing is
// always followed by a step.
bool dec_step_due(const cjs_bz_dec* d) {
  if (d->ended || d->pend_rc) return false;
  if (d->finished) return true;
  const size_t fresh = d->win_len - d->seen;
  return d->eager ? fresh > 0 : (fresh >= d->chunk || (d->win_len == d->win_cap && fresh > 0));
}

}  // namespace

extern "C" int cjs_bzip2_dec_create(cjs_bz_dec** out, int multistream, size_t chunk_bytes, size_t out_bytes, const cjs_opts* opts) {
  if (!out) return CJS_E_INVALID_ARG;
  *out = nullptr;
  CJS_GUARD_BEGIN
  cjs_bz_dec* d = new cjs_bz_dec();
  d->multistream = multistream ? 1 : 0;
  if (!chunk_bytes) {                      // the default; CJS_DEC_CHUNK_BYTES replaces it (callers without a chunk argument: the JS fronts, cli.js)
    const char* env = getenv("CJS_DEC_CHUNK_BYTES");
    chunk_bytes = env ? (size_t)strtoull(env, nullptr, 10) : 0;
    if (!chunk_bytes) chunk_bytes = DEC_DEFAULT_CHUNK;
  }
  d->chunk = std::min(std::max(chunk_bytes, DEC_MIN_CHUNK), DEC_MAX_CHUNK);
  d->out_req = out_bytes;
  d->device = Opts(opts).device;
  const char* eager = getenv("CJS_DEC_STREAM_EAGER");
  d->eager = eager && eager[0] == '1';
  d->debug = getenv("CJS_DEBUG") != nullptr;
  d->win_cap = d->chunk + (size_t)dec_extent(900000u);
  *out = d;
  return 0;
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

extern "C" int cjs_bzip2_dec_write(cjs_bz_dec* d, const uint8_t* in, size_t n, size_t* taken) {
  if (taken) *taken = 0;
  if (!d) return CJS_E_INVALID_ARG;
  if (d->rc) return d->fail(d->rc, nullptr);
  if (!taken || (!in && n) || d->finished) return d->fail(CJS_E_INVALID_ARG, nullptr);
  if (d->ended || d->pend_rc) { *taken = n; return 0; }      // the end has been decided: the reference never reads these bytes
  if (!n) return 0;
  if (!d->win && !(d->win = (uint8_t*)malloc(d->win_cap))) return d->fail(CJS_E_OUT_OF_MEMORY, nullptr);
  const size_t take = std::min(n, d->win_cap - d->win_len);
  memcpy(d->win + d->win_len, in, take);
  d->win_len += take; d->written += take;
  *taken = take;
  return 0;
}

extern "C" int cjs_bzip2_dec_finish(cjs_bz_dec* d) {
  if (!d) return CJS_E_INVALID_ARG;
  if (d->rc) return d->fail(d->rc, nullptr);
  d->finished = true;
  return 0;
}

extern "C" int cjs_bzip2_dec_read(cjs_bz_dec* d, uint8_t* out, size_t cap, size_t* got) {
  if (got) *got = 0;
  if (!d) return CJS_E_INVALID_ARG;
  if (d->rc) return d->fail(d->rc, nullptr);
  if (!got || (!out && cap)) return d->fail(CJS_E_INVALID_ARG, nullptr);
  CJS_GUARD_BEGIN
  for (;;) {
    if (d->held_pos < d->held) {
      const size_t take = std::min(cap, d->held - d->held_pos);
      if (take) memcpy(out, d->h_out.p + d->held_pos, take);
      d->held_pos += take;
      *got = take;
      return 0;
    }
    if (d->pend_rc) return d->fail(d->pend_rc, d->pend_detail);      // every byte in front of it has been read
    if (d->ended) return 0;
    if (!d->header_ok) {
      if (d->written < 4 && !d->finished) return 0;
      CJS_TRY(dec_header(d));
    }
    if (!dec_step_due(d)) return 0;
    if (!d->win && !(d->win = (uint8_t*)malloc(d->win_cap))) return d->fail(CJS_E_OUT_OF_MEMORY, nullptr);
    const int rc = dec_step(d);
    if (rc) return d->fail(rc, cjs_last_error_detail());
  }
  CJS_GUARD_END(d->fail(CJS_E_OUT_OF_MEMORY, nullptr), d->fail(CJS_E_HIP, nullptr))
}

extern "C" int cjs_bzip2_dec_done(const cjs_bz_dec* d) { return d && !d->rc && d->ended && d->held_pos == d->held ? 1 : 0; }

extern "C" void cjs_bzip2_dec_destroy(cjs_bz_dec* d) { delete d; }
