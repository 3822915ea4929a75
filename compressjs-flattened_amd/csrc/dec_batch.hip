// dec_batch.hip -- the decode engine's (dec_engine.h, decode.hip) batch drivers and its device-resident source and sink:
// cjs_bzip2_decompress_batch (Bzip2.decompressFiles), cjs_bzip2_decompress_device and cjs_bzip2_decompress_batch_device.
// (batch_dec.hip holds the batch form of block decode's kernels, dec_device.hip the kernels of the device-resident source.)
#include "dec_engine.h"
#include <memory>
#include <stdlib.h>
#include <string.h>

using namespace cjs;

// ---------------------------------------------------------------- batch group (host form: dec_batch_group, device form: dev_group_*)
// Inputs go in groups of up to BATCH_DEC_GROUP_BYTES, each group one upload with every input at a 4-byte-aligned offset and one
// share of phases A-C: one magic scan over the group (a candidate never straddles two inputs), block decode of all candidates
// with every read bounded by the candidate's own input, then the walk of each input over the candidates of its bytes, phase B
// over all chain blocks, phase C with a CRC verdict per block.  An input larger than a group goes through the single-stream
// path.  What the two forms share is here and in dec_engine.h (group_layout, group_prepare); where the bytes come from and where
// they go is theirs.  See DESIGN.md §6c.
namespace cjs {

constexpr size_t BATCH_DEC_GROUP_BYTES = (size_t)256 << 20;

size_t dec_group_bytes() {
  static const size_t g = getenv("CJS_DEC_GROUP_BYTES") ? (size_t)strtoull(getenv("CJS_DEC_GROUP_BYTES"), nullptr, 10) : BATCH_DEC_GROUP_BYTES;   // (tests shrink it)
  return g && g <= ((size_t)1 << 30) ? g : BATCH_DEC_GROUP_BYTES;      // (group offsets are 32-bit)
}

// the group that starts at input k0 (n[k0] <= G): inputs [k0, k1) whose 4-byte-aligned sizes come to G at most
size_t dec_group_end(const size_t* n, size_t count, size_t k0, size_t G) {
  size_t k1 = k0, bytes = 0;
  while (k1 < count && n[k1] <= G && (k1 == k0 || bytes + n[k1] <= G)) bytes += (n[k1++] + 3) & ~(size_t)3;
  return k1;
}

// After phase C (J.crc_got): input k's verdict is the single call's -- the first block of its chain, in stream order, whose CRC
// fails (:1756-1761); else what its header or its walk left in status / detail; else success -- and its bytes: off from `base`
// on, len 0 for a failed input.
void group_verdicts(const DecJob& J, const BatchGroup& G, size_t base, size_t* off, size_t* len, int32_t* status, std::vector<std::string>& detail) {
  for (size_t i = 0; i < G.k1 - G.k0; i++) {
    const size_t k = G.k0 + i;
    for (size_t b = G.ch0[i]; b < G.ch1[i]; b++) if (J.crc_got[b] != J.chain[b].crc) {
      char d[96];
      bad_crc_detail(d, sizeof d, J.crc_got[b], J.chain[b].crc);
      status[k] = CJS_E_DATA_ERROR; detail[k] = d;
      break;
    }
    off[k] = base + (size_t)J.out_off[G.ch0[i]];
    len[k] = status[k] ? 0 : (size_t)(J.out_off[G.ch1[i]] - J.out_off[G.ch0[i]]);
  }
}

bool on_device(const void* p, int dev) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
  return a.type == hipMemoryTypeDevice && a.device == dev;
}

}  // namespace cjs

// ---------------------------------------------------------------- device-resident source and sink (cjs_bzip2_decompress_device)
// bunzip_core with the input and the output in the GPU's memory.  The host path reads its host copy of the input in four places;
// each is a device pass here (dec_device.hip): the header (dd_headers, one 8-byte D2H), the level pre-scan of a multistream input
// (dd_level_scan: bz_max_level's rule), the upload (a device-to-device copy into phase A's dword-phased scratch) and, after the
// magic scan, the stored stream CRC and restart header of every end-of-stream candidate (dd_eos_bytes), which bz_walk reads
// through DevWalkBytes.  Phase C expands into the caller's buffer at the final offsets.  One share: the input lives on one GPU.
// See DESIGN.md §6d.
namespace {

// a single input's return code that is a failure of the whole batch call, not that input's verdict
bool fails_the_call(int r) { return r == CJS_E_OUT_OF_MEMORY || r == CJS_E_NO_DEVICE || r == CJS_E_HIP || r == CJS_E_INVALID_ARG; }

// what bz_walk reads of a device input: its 4 header bytes, and EOS_REC bytes from byte `at` on at the end-of-stream candidate
// the walk stands on
struct DevWalkBytes {
  const uint8_t* hdr; const uint8_t* rec = nullptr; uint64_t at = 0;
  uint8_t operator[](uint64_t i) const { if (rec && i - at < (uint64_t)EOS_REC) return rec[i - at]; return i < 4 ? hdr[i] : (uint8_t)0; }
};

// J->eos of a device source: EOS_REC bytes per end-of-stream candidate (rec_of[c]: its record, -1 for a block candidate)
int dev_eos_gather(DecShare* S, std::vector<uint8_t>& rec, std::vector<long>& rec_of) {
  const size_t nc = S->cands.size();
  std::vector<uint64_t> tab;
  rec_of.assign(nc, -1);
  for (size_t c = 0; c < nc; c++) if (S->cands[c].kind) {
    rec_of[c] = (long)(tab.size() / 2);
    tab.push_back((S->cands[c].bit + 48) >> 3);
    tab.push_back(S->bst.empty() ? S->up_hi : S->ben[S->cands[c].pad]);      // (a batch candidate: its own input's end)
  }
  const uint32_t ne = (uint32_t)(tab.size() / 2);
  rec.assign((size_t)ne * EOS_REC, 0);
  if (!ne) return 0;
  uint64_t* d_tab = nullptr; uint8_t* d_rec = nullptr;
  ShareScratch q(S);
  CJS_TRY(q.take((void**)&d_tab, 16 * (size_t)ne));
  CJS_TRY(q.take((void**)&d_rec, (size_t)ne * EOS_REC));
  if (hipMemcpyAsync(d_tab, tab.data(), 16 * (size_t)ne, hipMemcpyHostToDevice, S->s) != hipSuccess) return CJS_E_HIP;
  launch_dev_eos_bytes(S->s, S->d_in, d_tab, ne, d_rec);
  if (hipGetLastError() != hipSuccess || hipMemcpyAsync(rec.data(), d_rec, (size_t)ne * EOS_REC, hipMemcpyDeviceToHost, S->s) != hipSuccess ||
      hipStreamSynchronize(S->s) != hipSuccess) return CJS_E_HIP;
  S->h2d += 16 * (size_t)ne; S->d2h += (size_t)ne * EOS_REC;
  q.done();
  return 0;
}

// One decode of a device-resident source: a single stream (bunzip_core with one share) or a batch group (dec_batch_group).
// Prepared up to phase B, so that every size is known before anything is written, then emitted (phase C into the caller's buffer).
struct DevUnit {
  DecJob J;
  DecShare S;
  std::vector<uint8_t> rec; std::vector<long> rec_of;      // the end-of-stream candidates' bytes (dev_eos_gather)
  int pending = 0; char pending_detail[192] = {0};         // single: the walk's error, reported if every block in front passes its CRC
  uint64_t total = 0;                                       // bytes of the unit's output
  BatchGroup G;                                             // batch: inputs [G.k0, G.k1) of the call (a single stream of its own: one)
  std::vector<GatherPiece> pieces;                          // batch group: the gather of the inputs into the group layout
};

// _start_bunzip's bytes of `count` inputs (input k = d_in[off[k] .. off[k+1])), and for a multistream call the largest member level
// of each (bz_max_level), on S's stream and from its pool
int dev_headers(DecShare& S, const uint8_t* d_in, const std::vector<uint64_t>& off, bool multistream, std::vector<DevHdr>& hd) {
  const size_t count = off.size() - 1;
  hd.assign(count, DevHdr{});
  if (off.back() == off.front()) return 0;                       // (no bytes at all: every header is empty)
  if (hipSetDevice(S.device) != hipSuccess || (!S.s && hipStreamCreate(S.s.put()) != hipSuccess)) return CJS_E_HIP;
  uint64_t* d_off = nullptr; DevHdr* d_hdr = nullptr;
  ShareScratch q(&S);
  CJS_TRY(q.take((void**)&d_off, 8 * off.size()));
  CJS_TRY(q.take((void**)&d_hdr, sizeof(DevHdr) * count));
  if (hipMemcpyAsync(d_off, off.data(), 8 * off.size(), hipMemcpyHostToDevice, S.s) != hipSuccess) return CJS_E_HIP;
  launch_dev_headers(S.s, d_in, d_off, (uint32_t)count, multistream, off.front(), off.back(), d_hdr);
  if (hipGetLastError() != hipSuccess || hipMemcpyAsync(hd.data(), d_hdr, sizeof(DevHdr) * count, hipMemcpyDeviceToHost, S.s) != hipSuccess ||
      hipStreamSynchronize(S.s) != hipSuccess) return CJS_E_HIP;
  S.h2d += 8 * off.size(); S.d2h += sizeof(DevHdr) * count;
  q.done();
  return 0;
}

// the walk of one input over the candidates of its bytes (C.base: its first bit of the share's upload): the bytes behind an
// end-of-stream magic come from the candidate's record
int dev_walk(DevUnit& U, const WalkCands& C, const DevHdr& hd, size_t n, int multistream) {
  DevWalkBytes acc{hd.h};
  return walk_chain(U.J, C, acc, n, multistream, 0, [&](long ci, uint64_t pos) {
    if (C.kind(ci)) { acc.rec = U.rec.data() + (size_t)U.rec_of[(size_t)ci] * EOS_REC; acc.at = (pos + 48) >> 3; }
  });
}

// single stream, up to phase B: 0 (U.pending, U.total set) or what cjs_bzip2_decompress returns before its output stage
int dev_single_prepare(DevUnit& U, const uint8_t* d_in, size_t n, int multistream, const DevHdr& hd) {
  int level = 0; const char* why = nullptr;
  if (bz_header_check(hd.h, n, &level, &why)) { set_detail("%s", why); return CJS_E_NOT_BZIP_DATA; }
  DecJob& J = U.J; DecShare& S = U.S;
  J.n = n; J.mode = 0; J.timing = env_debug();
  J.tt_stride = 100000u * (uint32_t)(multistream ? std::max<int>(level, (int)hd.level) : level);
  J.upload = [d_in, n](DecShare* s, uint8_t* dst) { return hipMemcpyAsync(dst, d_in, n, hipMemcpyDeviceToDevice, s->s) != hipSuccess ? (int)CJS_E_HIP : 0; };
  J.eos = [&U](DecShare* s) { return dev_eos_gather(s, U.rec, U.rec_of); };
  S.lo = 0; S.hi = n; S.up_lo = 0; S.up_hi = n;
  guarded(S.rc, [&] { dec_phase_a(&J, &S); });
  if (S.rc) return S.rc;
  U.pending = dev_walk(U, WalkCands(&S, 1), hd, n, multistream);
  snprintf(U.pending_detail, sizeof U.pending_detail, "%s", cjs_last_error_detail());
  clear_detail();
  S.c0 = 0; S.c1 = J.chain.size();
  if (S.c1) {
    guarded(S.rc, [&] { dec_phase_b(&J, &S); });
    if (S.rc) return S.rc;
  }
  U.total = chain_out_offsets(J);
  return 0;
}

// single stream, phase C into d_out (nullptr: the CRC verdicts alone, in scratch; so with a pending error) -> the final verdict
int dev_single_emit(DevUnit& U, uint8_t* d_out) {
  if (!U.J.chain.empty()) {
    U.J.dev_out = U.pending ? nullptr : d_out; U.J.host = nullptr;
    U.S.rc = 0;
    guarded(U.S.rc, [&] { dec_phase_c(&U.J, &U.S); });
    if (U.S.rc) { if (U.S.detail[0]) set_detail("%s", U.S.detail); return U.S.rc; }
  }
  if (U.pending) { set_detail("%s", U.pending_detail); return U.pending; }
  return 0;
}

// a batch group up to phase B: the inputs (n[k] bytes from d_in + in_off[k] on, their headers in hd) are gathered into the group
// layout on the device, and a walk reads its bytes from hd and the end-of-stream records
int dev_group_prepare(DevUnit& U, const uint8_t* d_in, const size_t* in_off, const size_t* n, size_t k0, size_t k1, int multistream, const std::vector<DevHdr>& hd,
                      int32_t* status, std::vector<std::string>& detail) {
  DecJob& J = U.J;
  group_layout(J, U.S, U.G, k0, k1, n, status, detail, [&](size_t k) { return hd[k].h; },
               [&](size_t k, int level) { return multistream ? std::max<int>(level, (int)hd[k].level) : level; },
               [&](size_t k, size_t at) {
                 for (size_t p = 0; p < n[k]; p += GATHER_PIECE)      // (pieces of whole words: the last one of an input is zero-filled to one)
                   U.pieces.push_back(GatherPiece{in_off[k] + p, (uint32_t)(at + p), (uint32_t)std::min<size_t>(GATHER_PIECE, n[k] - p)});
               });
  J.upload = [&U, d_in](DecShare* s, uint8_t* dst) {
    GatherPiece* d_pc = nullptr;
    CJS_TRY(s->take((void**)&d_pc, sizeof(GatherPiece) * U.pieces.size()));
    if (hipMemcpyAsync(d_pc, U.pieces.data(), sizeof(GatherPiece) * U.pieces.size(), hipMemcpyHostToDevice, s->s) != hipSuccess) return (int)CJS_E_HIP;
    s->h2d += sizeof(GatherPiece) * U.pieces.size();
    launch_dev_gather(s->s, d_in, d_pc, (uint32_t)U.pieces.size(), dst);
    return hipGetLastError() != hipSuccess ? (int)CJS_E_HIP : 0;
  };
  J.eos = [&U](DecShare* s) { return dev_eos_gather(s, U.rec, U.rec_of); };
  return group_prepare(J, U.S, U.G, status, detail, [&](size_t k, const WalkCands& C) { return dev_walk(U, C, hd[k], n[k], multistream); }, &U.total);
}

// a batch group, phase C into d_out (the group's region): every input's status, offset (from d_out) and length
int dev_group_emit(DevUnit& U, uint8_t* d_out, size_t base, size_t* out_off, size_t* out_len, int32_t* status, std::vector<std::string>& detail) {
  DecJob& J = U.J;
  J.crc_got.assign(J.chain.size(), 0);
  J.dev_out = d_out;
  if (!J.chain.empty()) { U.S.rc = 0; guarded(U.S.rc, [&] { dec_phase_c(&J, &U.S); }); }
  if (U.S.rc) return U.S.rc;
  group_verdicts(J, U.G, base, out_off, out_len, status, detail);
  return 0;
}

}  // namespace

extern "C" int cjs_bzip2_decompress_device(const uint8_t* d_in, size_t n, int multistream, uint8_t* d_out, size_t out_cap, size_t* out_n, const cjs_opts* opts) {
  if (!out_n || (!d_in && n) || (!d_out && out_cap)) return CJS_E_INVALID_ARG;
  *out_n = 0;
  clear_detail();
  CJS_GUARD_BEGIN
  int dev = 0;
  CJS_TRY(current_device(opts, dev));
  RestoreDevice restore{dev};
  if ((n && !on_device(d_in, dev)) || (out_cap && !on_device(d_out, dev))) return CJS_E_INVALID_ARG;      // (no host pointer reaches a kernel)
  DevUnit U;
  U.S.device = dev;
  std::vector<DevHdr> hd;
  CJS_TRY(dev_headers(U.S, d_in, {0, (uint64_t)n}, multistream != 0, hd));
  int rc = dev_single_prepare(U, d_in, n, multistream, hd[0]);
  if (!rc && !U.pending && U.total > out_cap) { *out_n = (size_t)U.total; rc = CJS_E_OUTPUT_TOO_SMALL; }      // (d_out untouched)
  else if (!rc) rc = dev_single_emit(U, d_out);
  U.S.release();
  if (U.J.timing)
    fprintf(stderr, "[cjs dec dev] single: %zu bytes in, %llu bytes out, H2D %llu D2H %llu candidates %zu blocks %zu\n", n, (unsigned long long)U.total,
            (unsigned long long)U.S.h2d, (unsigned long long)U.S.d2h, U.S.cands.size(), U.J.chain.size());
  if (!rc) *out_n = (size_t)U.total;
  return rc;
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

// ---------------------------------------------------------------- batch (Bzip2.decompressFiles)
// The groups above with the inputs and the result in host memory: a group's inputs are staged into one host buffer and uploaded
// as phase A uploads a single stream; phase C copies the bytes back into a result buffer of the group.  See DESIGN.md §6c.
namespace {

struct BatchPiece { HostBuf buf; size_t size = 0; };       // a result buffer and the bytes used in it

// one group: inputs [k0, k1); every status / off (inside the group's piece) / len and detail is set
int dec_batch_group(const uint8_t* const* in, const size_t* n, size_t k0, size_t k1, int multistream, int dev, size_t* off, size_t* len,
                    int32_t* status, std::vector<std::string>& detail, BatchPiece* piece) {
  HostBuf host_in, result;                                     // (declared in front of the share: given back once its stream has drained)
  DecJob J; DecShare S; BatchGroup G;
  S.device = dev;
  for (size_t k = k0; k < k1; k++) off[k] = len[k] = 0;
  group_layout(J, S, G, k0, k1, n, status, detail, [&](size_t k) { return in[k]; },
               [&](size_t k, int level) { return bz_max_level(in[k], n[k], level, multistream != 0); }, [](size_t, size_t) {});
  host_in = HostBuf(J.n ? J.n : 1);
  if (!host_in) return CJS_E_OUT_OF_MEMORY;
  for (size_t k = k0; k < k1; k++) if (G.ok[k - k0]) memcpy(host_in.p + S.bst[k - k0], in[k], n[k]);
  J.in = host_in.p;
  uint64_t total = 0;
  CJS_TRY(group_prepare(J, S, G, status, detail, [&](size_t k, const WalkCands& C) { return walk_chain(J, C, in[k], n[k], multistream, 0, met_nothing); }, &total));
  const size_t nb = J.chain.size();
  result = HostBuf(total ? (size_t)total : 1);
  if (!(J.host = result.p)) return CJS_E_OUT_OF_MEMORY;
  J.crc_got.assign(nb, 0);
  if (nb) guarded(S.rc, [&] { dec_phase_c(&J, &S); });
  S.release();                                                 // (the stream has drained before J.host is read or given back)
  if (S.rc) return S.rc;
  group_verdicts(J, G, 0, off, len, status, detail);
  if (J.timing)
    fprintf(stderr, "[cjs dec batch] group: %zu inputs, %zu candidates, %u row batches (phase A), %u inverse-BWT batches (phase B), %zu chain blocks, %llu bytes out\n",
            k1 - k0, S.cands.size(), S.a_batches, S.b_batches, nb, (unsigned long long)total);
  piece->buf = std::move(result); piece->size = (size_t)total;
  return 0;
}

}  // namespace

extern "C" int cjs_bzip2_decompress_batch(const uint8_t* const* in, const size_t* n, size_t count, int multistream, uint8_t** out, size_t* off,
                                          size_t* len, int32_t* status, const cjs_opts* opts) {
  if (!out) return CJS_E_INVALID_ARG;
  *out = nullptr;
  clear_detail();
  if (count == 0) return 0;
  if (!in || !n || !off || !len || !status) return CJS_E_INVALID_ARG;
  for (size_t k = 0; k < count; k++) if (n[k] && !in[k]) return CJS_E_INVALID_ARG;
  CJS_GUARD_BEGIN
  int dev = 0;
  CJS_TRY(current_device(opts, dev));
  RestoreDevice restore{dev};
  cjs_opts one; memset(&one, 0, sizeof one);                   // (the large inputs: this device, n_devices and stats ignored)
  one.struct_size = sizeof one; one.device = dev;
  const size_t G = dec_group_bytes();
  std::vector<std::string> detail(count);
  std::vector<BatchPiece> pieces;                              // (every buffer goes back on every path out, but the one handed to the caller)
  std::vector<size_t> piece_of(count);
  int rc = 0;
  for (size_t k0 = 0; k0 < count && !rc;) {
    if (n[k0] > G) {                                           // an input of its own: the single-stream path
      uint8_t* o = nullptr; size_t on = 0;
      const int r = cjs_bzip2_decompress(in[k0], n[k0], multistream, &o, &on, &one);
      if (fails_the_call(r)) { rc = r; break; }
      status[k0] = r; off[k0] = 0; len[k0] = r ? 0 : on;
      if (r) detail[k0] = cjs_last_error_detail();
      piece_of[k0] = pieces.size();
      pieces.emplace_back();
      if (!r) { pieces.back().buf.reset(o); pieces.back().size = on; }
      k0++;
      continue;
    }
    const size_t k1 = dec_group_end(n, count, k0, G);
    pieces.emplace_back();
    if ((rc = dec_batch_group(in, n, k0, k1, multistream, dev, off, len, status, detail, &pieces.back())) != 0) break;
    for (size_t k = k0; k < k1; k++) piece_of[k] = pieces.size() - 1;
    k0 = k1;
  }
  clear_detail();
  if (rc) return rc;
  uint8_t* res = nullptr;
  if (pieces.size() == 1 && pieces[0].buf) res = pieces[0].buf.release();      // (one group: its buffer is the result)
  else {
    std::vector<size_t> base(pieces.size() + 1, 0);
    for (size_t i = 0; i < pieces.size(); i++) base[i + 1] = base[i] + pieces[i].size;
    if (!(res = (uint8_t*)HostPool::take(base.back() ? base.back() : 1))) return CJS_E_OUT_OF_MEMORY;
    for (size_t i = 0; i < pieces.size(); i++) if (pieces[i].size) memcpy(res + base[i], pieces[i].buf.p, pieces[i].size);
    for (size_t k = 0; k < count; k++) off[k] += base[piece_of[k]];
  }
  *out = res;
  for (size_t k = 0; k < count; k++) if (status[k]) { set_detail("%s", detail[k].c_str()); break; }      // the lowest-index failing input's
  return 0;
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

// ---------------------------------------------------------------- device-resident batch (cjs_bzip2_decompress_batch_device)
// cjs_bzip2_decompress_batch with the inputs and the result in GPU memory: the same groups (dec_group_bytes), verdicts and layout.
// Every group and every input above the group size (the single device path) is prepared up to phase B first -- the single
// ones also through a CRC-only phase C, as a failed one takes no bytes -- so the layout and its size are known before anything
// is written; then each emits into its region of d_out.  See DESIGN.md §6d.
extern "C" int cjs_bzip2_decompress_batch_device(const uint8_t* d_in, const size_t* in_off, size_t count, int multistream, uint8_t* d_out, size_t out_cap,
                                                 size_t* out_off, size_t* out_len, int32_t* status, size_t* out_need, const cjs_opts* opts) {
  clear_detail();
  if (count == 0) { if (out_need) *out_need = 0; return 0; }
  if (!in_off || !out_off || !out_len || !status || !out_need || count >= 0xFFFFFFFFu) return CJS_E_INVALID_ARG;
  for (size_t k = 0; k < count; k++) if (in_off[k + 1] < in_off[k]) return CJS_E_INVALID_ARG;
  if ((!d_in && in_off[count] > in_off[0]) || (!d_out && out_cap)) return CJS_E_INVALID_ARG;
  *out_need = 0;
  CJS_GUARD_BEGIN
  int dev = 0;
  CJS_TRY(current_device(opts, dev));
  RestoreDevice restore{dev};
  if ((in_off[count] > in_off[0] && !on_device(d_in + in_off[0], dev)) || (out_cap && !on_device(d_out, dev))) return CJS_E_INVALID_ARG;
  DecShare H;                                                   // the header pass: its stream, pool and copy tally
  H.device = dev;
  std::vector<DevHdr> hd;
  CJS_TRY(dev_headers(H, d_in, std::vector<uint64_t>(in_off, in_off + count + 1), multistream != 0, hd));
  H.release();
  const size_t G = dec_group_bytes();
  std::vector<size_t> n(count);
  for (size_t k = 0; k < count; k++) n[k] = in_off[k + 1] - in_off[k];
  std::vector<std::string> detail(count);
  std::vector<std::unique_ptr<DevUnit>> units;
  std::vector<size_t> unit_base;
  uint64_t need = 0;
  for (size_t k0 = 0; k0 < count;) {
    units.emplace_back(new DevUnit);
    DevUnit& U = *units.back();
    U.S.device = dev;
    if (n[k0] > G) {                                            // an input of its own: the single device path
      U.G.k0 = k0; U.G.k1 = k0 + 1;
      clear_detail();
      int r = dev_single_prepare(U, d_in + in_off[k0], n[k0], multistream, hd[k0]);
      if (!r) r = dev_single_emit(U, nullptr);                  // (the verdict: a failed input takes no bytes)
      if (fails_the_call(r)) return r;
      status[k0] = r;
      if (r) { detail[k0] = cjs_last_error_detail(); U.S.release(); }
      unit_base.push_back((size_t)need);
      out_off[k0] = (size_t)need; out_len[k0] = r ? 0 : (size_t)U.total;
      need += r ? 0 : U.total;
      k0++;
      continue;
    }
    const size_t k1 = dec_group_end(n.data(), count, k0, G);
    CJS_TRY(dev_group_prepare(U, d_in, in_off, n.data(), k0, k1, multistream, hd, status, detail));
    unit_base.push_back((size_t)need);
    need += U.total;
    k0 = k1;
  }
  clear_detail();
  *out_need = (size_t)need;
  uint64_t h2d = H.h2d, d2h = H.d2h, cands = 0, blocks = 0;
  auto tally = [&]() {
    for (auto& u : units) { h2d += u->S.h2d; d2h += u->S.d2h; cands += u->S.cands.size(); blocks += u->J.chain.size(); }
    if (env_debug())
      fprintf(stderr, "[cjs dec dev] batch: %zu inputs, %zu units, %llu bytes out, H2D %llu D2H %llu candidates %llu blocks %llu\n", count, units.size(),
              (unsigned long long)need, (unsigned long long)h2d, (unsigned long long)d2h, (unsigned long long)cands, (unsigned long long)blocks);
  };
  if (need > out_cap) { tally(); return CJS_E_OUTPUT_TOO_SMALL; }      // (d_out untouched)
  for (size_t u = 0; u < units.size(); u++) {
    DevUnit& U = *units[u];
    if (U.J.batch) CJS_TRY(dev_group_emit(U, d_out + unit_base[u], unit_base[u], out_off, out_len, status, detail));
    else if (!status[U.G.k0] && dev_single_emit(U, d_out + unit_base[u]) != 0) return CJS_E_HIP;      // (its verdict was 0 a moment ago)
    U.S.release();
  }
  tally();
  clear_detail();
  for (size_t k = 0; k < count; k++) if (status[k]) { set_detail("%s", detail[k].c_str()); break; }      // the lowest-index failing input's
  return 0;
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}
