// dec_recover.hip -- recovery of damaged .bz2 data (cjs_bzip2_recover[_device], no reference equivalent: the job of bzip2recover).
// Phases A, B and C of the decode engine (dec_engine.h, decode.hip) without the chain walk: one share over the whole input with rows
// sized for level 9 and no header check; every
// decodable block candidate becomes a "chain" block of phases B and C, which return a CRC verdict per block (DecJob::batch); the
// host then picks the survivors in ascending order (the rule: include/cjs_hip.h).  Phases B and C run over one inverse-BWT batch
// of the candidates at a time (dec_scratch_batches), phase C expanding into scratch of the batch's size, and only the survivors leave
// it: so the memory held is phase A's (the upload and the decoded rows, as for decompression) plus one batch's, however many
// candidates there are.  The stream form gathers the survivors' bit strings from the upload, which stays with the share, into a
// zeroed buffer of the new stream's size (bz_bits_gather).  See DESIGN.md §6g.
#include "dec_engine.h"
#include <stdlib.h>
#include <string.h>

using namespace cjs;

namespace cjs {

// Bits [src_bit, src_bit + nbits) of a source go to bits [dst_bit, ..) of `out`; bit b of either is bit 31 - (b & 31) of the
// big-endian 32-bit word b >> 5.  src: the device address of the source's word 0 (4-byte aligned), src_words: the words of it
// that may be read.  nbits >= 1.
struct BitRun { uint64_t src, src_words, src_bit, dst_bit, nbits; };
// One thread per DESTINATION word of a run (workgroups along grid.x stride over the run's words, grid.y = the runs of a slab):
// the two source words the word straddles, a funnel shift, and the mask of the destination bits that are the run's -- what lies
// in front of the first and behind the last source bit belongs to other blocks or to damage.  A word wholly inside its run is
// stored; the first and the last word of a run, which two runs may share, are ORed into the zeroed buffer.
__global__ __launch_bounds__(256) void bz_bits_gather(const BitRun* __restrict__ runs, uint32_t run0, uint32_t* __restrict__ out) {
  const BitRun r = runs[run0 + blockIdx.y];
  const uint32_t* __restrict__ src = reinterpret_cast<const uint32_t*>(r.src);
  const uint64_t d1 = r.dst_bit + r.nbits, w0 = r.dst_bit >> 5, w1 = (d1 - 1) >> 5;
  for (uint64_t w = w0 + (uint64_t)blockIdx.x * 256 + threadIdx.x; w <= w1; w += (uint64_t)gridDim.x * 256) {
    const int64_t t = (int64_t)r.src_bit + ((int64_t)(w << 5) - (int64_t)r.dst_bit);      // the source bit that lands on the word's first bit
    const int64_t wi = t >> 5;                                                              // (floor: t >= -31)
    const uint32_t sh = (uint32_t)(t & 31);
    const uint32_t hi = wi >= 0 && (uint64_t)wi < r.src_words ? __builtin_bswap32(src[wi]) : 0u;
    const uint32_t lo = sh && wi + 1 >= 0 && (uint64_t)(wi + 1) < r.src_words ? __builtin_bswap32(src[wi + 1]) : 0u;
    uint32_t v = sh ? __builtin_amdgcn_alignbit(hi, lo, 32u - sh) : hi;
    const uint32_t a = w == w0 ? (uint32_t)(r.dst_bit & 31) : 0u, b = w == w1 ? (uint32_t)((d1 - 1) & 31) + 1u : 32u;      // the run's bits [a, b) of the word
    const uint32_t mask = (0xFFFFFFFFu >> a) & (b == 32u ? 0xFFFFFFFFu : ~(0xFFFFFFFFu >> b));
    v = __builtin_bswap32(v & mask);
    if (mask == 0xFFFFFFFFu) out[w] = v; else atomicOr(&out[w], v);
  }
}

}  // namespace cjs

namespace {

// the recovered bytes on the host: a HostPool buffer that grows batch by batch (one batch -- the usual case -- never copies)
struct RecHost {
  HostBuf buf; size_t cap = 0;
  int ensure(size_t used, size_t need) {
    if (need <= cap && buf) return 0;
    const size_t nc = std::max<size_t>(std::max<size_t>(need, 2 * cap), 1);
    HostBuf q(nc);
    if (!q) return CJS_E_OUT_OF_MEMORY;
    if (used) memcpy(q.p, buf.p, used);
    buf = std::move(q); cap = nc;
    return 0;
  }
};

// in: the input on the host, or nullptr with d_src: the input on device `dev`.  host_out: the host form's result; else d_out /
// out_cap (checked by the caller).  found / cap / n_found as in the C ABI.
int recover_core(const uint8_t* in, const uint8_t* d_src, size_t n, bool as_stream, uint8_t** host_out, uint8_t* d_out, size_t out_cap, size_t* out_n,
                 cjs_bz_found* found, long cap, long* n_found, int dev) {
  RecHost host;                                                   // (declared first: given back after the share's stream has drained)
  DecJob J; DecShare S;
  J.in = in; J.n = n; J.mode = 0; J.batch = true; J.timing = env_debug();
  J.tt_stride = 900000u;
  if (d_src) J.upload = [d_src, n](DecShare* s, uint8_t* dst) { return hipMemcpyAsync(dst, d_src, n, hipMemcpyDeviceToDevice, s->s) != hipSuccess ? (int)CJS_E_HIP : 0; };
  S.device = dev; S.lo = 0; S.hi = n; S.up_lo = 0; S.up_hi = n;
  guarded(S.rc, [&] { dec_phase_a(&J, &S); });
  if (S.rc) return S.rc;
  hipStream_t s = S.s;

  std::vector<uint32_t> bc;                                       // the block candidates (indices into S.cands), ascending
  for (uint32_t c = 0; c < S.cands.size(); c++) if (S.cands[c].kind == 0) bc.push_back(c);
  const size_t nc = bc.size();
  *n_found = (long)nc;
  const uint64_t nbits = (uint64_t)n * 8;
  std::vector<uint32_t> chain_bc;                                 // chain block k is block candidate chain_bc[k]
  for (size_t i = 0; i < nc; i++) {
    const BlockOut& bo = S.bos[bc[i]];
    if (bo.err || bo.end_bit >= nbits) continue;                  // (the decoder clamps end_bit to the end: a block that touches it may have been cut off)
    J.chain.push_back(ib_block(bo, S.tt_ptr[bc[i]])); chain_bc.push_back((uint32_t)i);
  }
  const size_t nb = J.chain.size();

  std::vector<BitRun> runs;                                       // stream form: header, survivors, trailer
  uint64_t total = 0, last_end = 0, sbit = 32;                    // bytes recovered so far / the selection's state / the new stream's next bit
  uint32_t fold = 0;
  const uint64_t src_addr = (uint64_t)(uintptr_t)S.d_in, src_words = ((uint64_t)n + 3) / 4;      // (the upload has 256 bytes of slack)
  size_t next = 0;                                                // block candidates in front of `next` have their entry
  auto entry = [&](size_t i, int status, uint64_t end_bit, uint64_t off, uint32_t size) {
    if (!found || (long)i >= cap) return;
    cjs_bz_found& f = found[i];
    f.bitpos = S.cands[bc[i]].bit; f.end_bit = end_bit; f.out_off = off; f.size = size; f.status = status; f.crc = S.bos[bc[i]].crc; f.reserved = 0;
  };
  auto lost_upto = [&](size_t i1) {                               // the candidates that are not decodable, up to i1
    for (; next < i1; next++) {
      const BlockOut& bo = S.bos[bc[next]];
      entry(next, S.cands[bc[next]].bit < last_end ? CJS_REC_SHADOWED : bo.err ? bo.err : CJS_E_DATA_ERROR, 0, 0, 0);
    }
  };
  // the selection over a decoded batch, and the survivors' bytes as runs of neighbours in the scratch
  auto select = [&](size_t g0, size_t g1, uint8_t* d_exp, ShareScratch&) {
    struct Piece { uint64_t from, to, len; };
    std::vector<Piece> pieces;
    for (size_t k = g0; k < g1; k++) {
      const size_t i = chain_bc[k];
      lost_upto(i);
      const uint64_t p = S.cands[bc[i]].bit, e = S.bos[bc[i]].end_bit;
      next = i + 1;
      if (p < last_end) { entry(i, CJS_REC_SHADOWED, e, 0, 0); continue; }
      if (J.crc_got[k] != J.chain[k].crc) { entry(i, CJS_E_DATA_ERROR, e, 0, 0); continue; }
      const uint32_t len = J.chain[k].out_len;
      entry(i, 0, e, as_stream ? sbit : total, len);
      last_end = e;
      if (as_stream) {
        runs.push_back(BitRun{src_addr, src_words, p, sbit, e - p});
        sbit += e - p;
        fold = crc_fold(fold, J.chain[k].crc);
      } else if (len) {
        if (!pieces.empty() && pieces.back().from + pieces.back().len == J.out_off[k]) pieces.back().len += len;
        else pieces.push_back(Piece{J.out_off[k], total, len});
      }
      total += len;
    }
    if (as_stream || pieces.empty()) return 0;
    if (host_out) CJS_TRY(host.ensure((size_t)pieces[0].to, (size_t)total));
    for (const Piece& q : pieces) {
      hipError_t e = hipSuccess;
      if (host_out) e = hipMemcpyAsync(host.buf.p + q.to, d_exp + q.from, (size_t)q.len, hipMemcpyDeviceToHost, s);
      else if (q.to + q.len <= out_cap) e = hipMemcpyAsync(d_out + q.to, d_exp + q.from, (size_t)q.len, hipMemcpyDeviceToDevice, s);      // (what does not fit is only counted)
      if (e != hipSuccess) return (int)CJS_E_HIP;
      if (host_out) S.d2h += q.len;
    }
    return hipStreamSynchronize(s) != hipSuccess ? (int)CJS_E_HIP : 0;
  };
  CJS_TRY(dec_scratch_batches(J, S, select));
  lost_upto(nc);

  if (as_stream) {
    // header and trailer are two more runs, from a 16-byte source of their own: 'BZh9', then the end magic and the combined CRC
    uint8_t ht[16] = {'B', 'Z', 'h', '9', 0x17, 0x72, 0x45, 0x38, 0x50, 0x90, (uint8_t)(fold >> 24), (uint8_t)(fold >> 16), (uint8_t)(fold >> 8), (uint8_t)fold, 0, 0};
    const uint64_t sbits = sbit + 80;
    total = (sbits + 7) / 8;
    const size_t words = (size_t)((sbits + 31) / 32);
    uint8_t* d_ht = nullptr; BitRun* d_runs = nullptr; uint32_t* d_str = nullptr;
    CJS_TRY(S.take((void**)&d_ht, 16));
    runs.push_back(BitRun{(uint64_t)(uintptr_t)d_ht, 4, 0, 0, 32});
    runs.push_back(BitRun{(uint64_t)(uintptr_t)d_ht, 4, 32, sbit, 80});
    CJS_TRY(S.take((void**)&d_runs, sizeof(BitRun) * runs.size()));
    CJS_TRY(S.take((void**)&d_str, 4 * words));
    if (hipMemcpyAsync(d_ht, ht, 16, hipMemcpyHostToDevice, s) != hipSuccess || hipMemcpyAsync(d_runs, runs.data(), sizeof(BitRun) * runs.size(), hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemsetAsync(d_str, 0, 4 * words, s) != hipSuccess) return CJS_E_HIP;
    S.h2d += 16 + sizeof(BitRun) * runs.size();
    for (size_t r0 = 0; r0 < runs.size(); r0 += 65535) {          // (grid.y)
      const uint32_t nr = (uint32_t)std::min<size_t>(65535, runs.size() - r0);
      uint64_t mx = 0;
      for (size_t r = r0; r < r0 + nr; r++) mx = std::max(mx, runs[r].nbits);
      const uint32_t gx = (uint32_t)std::min<uint64_t>(256, (mx / 32 + 2 + 255) / 256);
      hipLaunchKernelGGL(bz_bits_gather, dim3(gx, nr), dim3(256), 0, s, d_runs, (uint32_t)r0, d_str);
    }
    if (hipGetLastError() != hipSuccess) return CJS_E_HIP;
    hipError_t e = hipSuccess;
    if (host_out) {
      CJS_TRY(host.ensure(0, (size_t)total));
      e = hipMemcpyAsync(host.buf.p, d_str, (size_t)total, hipMemcpyDeviceToHost, s);
      S.d2h += total;
    } else if (total <= out_cap) e = hipMemcpyAsync(d_out, d_str, (size_t)total, hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return CJS_E_HIP;
  }
  S.release();
  if (J.timing)
    fprintf(stderr, "[cjs recover] %zu bytes in, %zu candidates, %zu decodable, %u row batches (phase A), %u inverse-BWT batches, %llu bytes out (%s), H2D %llu D2H %llu\n", n, nc, nb,
            S.a_batches, S.b_batches, (unsigned long long)total, as_stream ? "stream" : "bytes", (unsigned long long)S.h2d, (unsigned long long)S.d2h);
  *out_n = (size_t)total;
  if (host_out) {
    CJS_TRY(host.ensure(0, 1));                                  // (nothing recovered: still a buffer, as cjs_bzip2_decompress gives)
    *host_out = host.buf.release();
    return 0;
  }
  return total > out_cap ? (int)CJS_E_OUTPUT_TOO_SMALL : 0;
}

// the stream form of "nothing found" (n < 6: no device needed)
const uint8_t REC_EMPTY_STREAM[14] = {'B', 'Z', 'h', '9', 0x17, 0x72, 0x45, 0x38, 0x50, 0x90, 0, 0, 0, 0};

}  // namespace

extern "C" int cjs_bzip2_recover(const uint8_t* in, size_t n, int as_stream, uint8_t** out, size_t* out_n, cjs_bz_found* found, long cap, long* n_found,
                                 const cjs_opts* opts) {
  if (!out || !out_n || !n_found || (!in && n) || (!found && cap > 0)) return CJS_E_INVALID_ARG;
  *out = nullptr; *out_n = 0; *n_found = 0;
  clear_detail();
  CJS_GUARD_BEGIN
  if (n < 6) {
    const size_t sz = as_stream ? sizeof REC_EMPTY_STREAM : 0;
    if (!(*out = (uint8_t*)malloc(sz ? sz : 1))) return CJS_E_OUT_OF_MEMORY;
    if (sz) memcpy(*out, REC_EMPTY_STREAM, sz);
    *out_n = sz;
    return 0;
  }
  int dev = 0;
  CJS_TRY(current_device(opts, dev));
  RestoreDevice restore{dev};
  const int rc = recover_core(in, nullptr, n, as_stream != 0, out, nullptr, 0, out_n, found, cap, n_found, dev);
  if (rc) { *out_n = 0; *n_found = 0; }
  return rc;
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

extern "C" int cjs_bzip2_recover_device(const uint8_t* d_in, size_t n, int as_stream, uint8_t* d_out, size_t out_cap, size_t* out_n, cjs_bz_found* found, long cap,
                                        long* n_found, const cjs_opts* opts) {
  if (!out_n || !n_found || (!d_in && n) || (!d_out && out_cap) || (!found && cap > 0)) return CJS_E_INVALID_ARG;
  *out_n = 0; *n_found = 0;
  clear_detail();
  CJS_GUARD_BEGIN
  if (n < 6 && !as_stream) return 0;
  int dev = 0;
  CJS_TRY(current_device(opts, dev));
  RestoreDevice restore{dev};
  if ((n && !on_device(d_in, dev)) || (out_cap && !on_device(d_out, dev))) return CJS_E_INVALID_ARG;      // (no host pointer reaches a kernel)
  if (n < 6) {                                                    // the empty stream
    *out_n = sizeof REC_EMPTY_STREAM;
    if (out_cap < sizeof REC_EMPTY_STREAM) return CJS_E_OUTPUT_TOO_SMALL;
    return hipMemcpy(d_out, REC_EMPTY_STREAM, sizeof REC_EMPTY_STREAM, hipMemcpyHostToDevice) != hipSuccess ? (int)CJS_E_HIP : 0;
  }
  const int rc = recover_core(nullptr, d_in, n, as_stream != 0, nullptr, d_out, out_cap, out_n, found, cap, n_found, dev);
  if (rc && rc != CJS_E_OUTPUT_TOO_SMALL) { *out_n = 0; *n_found = 0; }
  return rc;
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}
