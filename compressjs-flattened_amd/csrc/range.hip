// range.hip -- the indexed range reads (cjs_bzip2_index_build, cjs_bzip2_read_ranges[_device]): their two kernels
// and, on the decode engine (dec_engine.h, decode.hip), the pass engine with what its consumers share on the host
// (range_engine.h lists the four and the shared pieces), and the range reads' own consumer of it.
//   rg_slices       the slice gather: every piece (source address, destination address, length) of a pass in one launch per slab.
//                   It moves the ranges' bytes out of a pass's expanded blocks (to the packed device buffer of the host form, or
//                   straight into the caller's d_out), and it is the device form's upload: the byte runs of the touched blocks,
//                   out of the caller's d_in into the pass's upload buffer.
//   rg_cand_magic   the 48-bit block magic at every candidate the index names (there is no magic scan on this path)
#include "range_engine.h"
#include <algorithm>
#include <stdlib.h>
#include <string.h>

using namespace cjs;

namespace cjs {

// A slice = len bytes (1 .. SLICE_TASK) from device address src to device address dst, any alignment; n slices in launches of
// SLICE_SLAB.
struct Slice { uint64_t src, dst, len; };
constexpr uint64_t SLICE_TASK = 65536;                 // (a multiple of 16)
constexpr size_t SLICE_SLAB = 65535;

// The interior of a piece: nvec 16-byte vectors, the destination da aligned, the source sa = 16 * q + 4 * K + m behind an aligned
// address.  Lane i stores vector i (consecutive lanes, consecutive 16 bytes) from the two aligned source vectors it straddles
// (rg_funnel16).  K and m are the same for every vector of the piece, so the choice is made once per workgroup.
template <int K>
__device__ __forceinline__ void rg_interior(uint64_t sa, uint64_t da, uint64_t nvec, uint32_t m, uint64_t lo, uint64_t hi) {
  for (uint64_t v = threadIdx.x; v < nvec; v += 256) *reinterpret_cast<uint4*>(da + 16 * v) = rg_funnel16<K>(sa + 16 * v, m, lo, hi);
}

// One workgroup per piece (at most SLICE_TASK bytes: the host cuts longer ones).  Source and destination are at any byte
// alignment, also relative to each other.  Bytes in front of the destination's first 16-byte boundary and behind its last are
// byte stores; everything between is aligned 16-byte stores.  Writes stay inside [dst, dst + len), reads inside [src, src + len).
__global__ __launch_bounds__(256) void rg_slices(const Slice* __restrict__ sl, uint32_t s0) {
  const Slice t = sl[s0 + blockIdx.x];
  const uint64_t s = t.src, d = t.dst, len = t.len;
  const uint32_t head = (uint32_t)min(len, (0ull - d) & 15ull);
  const uint64_t nvec = (len - head) >> 4;
  const uint32_t tail = (uint32_t)((len - head) & 15u);
  if (threadIdx.x < head) *reinterpret_cast<uint8_t*>(d + threadIdx.x) = *reinterpret_cast<const uint8_t*>(s + threadIdx.x);
  if (threadIdx.x < tail) {
    const uint64_t o = head + 16 * nvec + threadIdx.x;
    *reinterpret_cast<uint8_t*>(d + o) = *reinterpret_cast<const uint8_t*>(s + o);
  }
  if (!nvec) return;
  const uint64_t sa = s + head, da = d + head;
  const uint32_t m = (uint32_t)(sa & 3u);
  switch ((uint32_t)(sa & 15u) >> 2) {
    case 0: rg_interior<0>(sa, da, nvec, m, s, s + len); break;
    case 1: rg_interior<1>(sa, da, nvec, m, s, s + len); break;
    case 2: rg_interior<2>(sa, da, nvec, m, s, s + len); break;
    default: rg_interior<3>(sa, da, nvec, m, s, s + len); break;
  }
}

// ok[c] = the 48 bits at bits[c] of `in` (n bytes) are the block magic, wholly inside the n bytes
__global__ __launch_bounds__(256) void rg_cand_magic(const uint8_t* __restrict__ in, uint64_t n, const uint64_t* __restrict__ bits, uint32_t nc, uint32_t* __restrict__ ok) {
  const uint32_t c = blockIdx.x * 256 + threadIdx.x;
  if (c >= nc) return;
  const uint64_t bit = bits[c], byte = bit >> 3;
  uint64_t w = 0;
  for (int i = 0; i < 7; i++) w = (w << 8) | (byte + i < n ? in[byte + i] : 0);      // 56 bits
  const uint64_t v = (w >> (8 - (bit & 7))) & 0xFFFFFFFFFFFFull;
  ok[c] = (bit + 48 <= n * 8 && v == MAGIC_BLOCK) ? 1u : 0u;
}

}  // namespace cjs

// ---------------------------------------------------------------- the driver
// recover_core's shape (dec_recover.hip) with the candidates given by an index instead of found by the scan: the blocks that the
// ranges touch go through phases A, B and C in ascending passes, a pass being what one upload of the batch decoder's group size
// holds.  Only the byte runs of a pass's blocks are uploaded, packed (RangeUpload), and phase A is told its candidates
// (DecJob::given): no magic scan, no stream header, no chain walk -- a block stands or falls by its own index entry.  Phase C expands a batch of
// blocks into scratch (dec_scratch_batches), where their CRCs are computed; the engine hands the batch to its consumer there: the
// slice gather takes every piece of every range from there to its place (range_run), the scan looks for patterns (search.hip).
namespace {

void launch_slices(hipStream_t s, const Slice* d_sl, size_t n) {
  for (size_t s0 = 0; s0 < n; s0 += SLICE_SLAB) hipLaunchKernelGGL(rg_slices, dim3((unsigned)std::min(SLICE_SLAB, n - s0)), dim3(256), 0, s, d_sl, (uint32_t)s0);
}
// ok[c] = the block magic stands at bit bits[c] of d_in (n bytes)
void launch_cand_magic(hipStream_t s, const uint8_t* d_in, uint64_t n, const uint64_t* d_bits, uint32_t nc, uint32_t* d_ok) {
  if (nc) hipLaunchKernelGGL(rg_cand_magic, dim3((nc + 255) / 256), dim3(256), 0, s, d_in, n, d_bits, nc, d_ok);
}

struct RangePiece { uint32_t block, in_off, len, pad; uint64_t out; };      // len bytes from byte in_off of the block to byte `out` of the layout

// What the index alone says about a call: the layout (lay_off / lay_len: range k clipped, packed in range order), the pieces
// sorted by block and the touched blocks, ascending.
struct RangePlan {
  std::vector<uint64_t> lay_off, lay_len;
  std::vector<RangePiece> pieces;
  std::vector<uint32_t> touched;
  uint64_t total = 0;
};

int range_plan(const cjs_bz_index* ix, const uint64_t* off, const uint64_t* len, size_t count, RangePlan& P) {
  const uint64_t end = ix->off.back();
  P.lay_off.assign(count, 0); P.lay_len.assign(count, 0);
  for (size_t k = 0; k < count; k++) {
    if (off[k] + len[k] < off[k]) { set_detail("range %zu: offset + length overflows", k); return CJS_E_INVALID_ARG; }
    P.lay_off[k] = P.total;
    if (off[k] >= end || !len[k]) continue;
    P.lay_len[k] = std::min<uint64_t>(len[k], end - off[k]);
    uint64_t pos = off[k], left = P.lay_len[k];
    for (size_t b = range_block_of(ix, pos); left; b++) {
      const uint64_t take = std::min<uint64_t>(left, ix->off[b + 1] - pos);
      if (take) P.pieces.push_back(RangePiece{(uint32_t)b, (uint32_t)(pos - ix->off[b]), (uint32_t)take, 0u, P.total + (pos - off[k])});
      pos += take; left -= take;
    }
    P.total += P.lay_len[k];
  }
  std::stable_sort(P.pieces.begin(), P.pieces.end(), [](const RangePiece& a, const RangePiece& b) { return a.block < b.block; });
  for (const RangePiece& p : P.pieces) if (P.touched.empty() || P.touched.back() != p.block) P.touched.push_back(p.block);
  return 0;
}

// One pass's upload: the byte runs [bitpos >> 3, (end_bit + 7) >> 3) of touched blocks [t0, t1), neighbours merged, each run at a
// packed offset congruent to its source address mod 16 (the device gather then stores aligned vectors from aligned vectors).
struct RangeRun { uint64_t lo, hi, at; };      // stream bytes [lo, hi) at byte `at` of the upload
struct RangeUpload {
  std::vector<RangeRun> runs; std::vector<uint64_t> bit;      // bit[i]: where touched block t0 + i's magic starts in the upload
  uint64_t bytes = 0;
  uint64_t bytes_with(const cjs_bz_index_entry& e, uint64_t src_addr) const {      // `bytes` once e has been added
    const uint64_t lo = e.bitpos >> 3, hi = (e.end_bit + 7) >> 3;
    if (runs.empty() || lo > runs.back().hi) return ((bytes + 15) & ~15ull) + ((src_addr + lo) & 15u) + (hi - lo);
    return runs.back().at + (std::max(runs.back().hi, hi) - runs.back().lo);
  }
  void add(const cjs_bz_index_entry& e, uint64_t src_addr) {
    const uint64_t lo = e.bitpos >> 3, hi = (e.end_bit + 7) >> 3;
    if (runs.empty() || lo > runs.back().hi) {
      const uint64_t at = ((bytes + 15) & ~15ull) + ((src_addr + lo) & 15u);
      runs.push_back(RangeRun{lo, hi, at});
    } else runs.back().hi = std::max(runs.back().hi, hi);
    bytes = runs.back().at + (runs.back().hi - runs.back().lo);
    bit.push_back((runs.back().at - runs.back().lo) * 8 + e.bitpos);
  }
};

constexpr uint64_t RANGE_PASS_DECODED = 4ull << 30;      // decoded bytes of a pass by the index (what phase A keeps of it is at most 1.25 x that)

size_t range_pass_blocks() {      // (read at every call: tests run the several-pass path at small sizes)
  const char* v = getenv("CJS_RANGE_PASS_BLOCKS");
  const unsigned long long x = v ? strtoull(v, nullptr, 10) : 0;
  return x ? (size_t)x : ~(size_t)0;
}

// slices of one piece of `len` bytes, cut where the destination crosses a multiple of SLICE_TASK behind its first 16-byte boundary
void range_slices(std::vector<Slice>& sl, uint64_t src, uint64_t dst, uint64_t len) {
  uint64_t cut = std::min<uint64_t>(len, SLICE_TASK - (dst & 15u));
  for (uint64_t o = 0; o < len; cut = std::min<uint64_t>(len - o, SLICE_TASK)) { sl.push_back(Slice{src + o, dst + o, cut}); o += cut; }
}

}  // namespace

// The pass engine (range_engine.h): the passes over `touched`, each block's verdict, every decoded batch handed to `consume`.
int cjs::range_engine(const uint8_t* in, const uint8_t* d_src, const cjs_bz_index* ix, const std::vector<uint32_t>& touched, RangeVerdicts& V, int dev,
                      RangeStats& st, const RangeConsumer& consume) {
  const size_t nt = touched.size(), cap_blocks = range_pass_blocks(), G = dec_group_bytes();
  Stream keep;                                                     // one stream for all passes
  for (size_t t0 = 0; t0 < nt;) {
    // ---- the pass: touched blocks [t0, t1)
    RangeUpload U;
    size_t t1 = t0; uint32_t max_level = 1; uint64_t decoded = 0;
    while (t1 < nt && t1 - t0 < cap_blocks && t1 - t0 < DEC_BATCH_BLOCKS) {
      const cjs_bz_index_entry& e = ix->e[touched[t1]];
      if (t1 > t0 && (U.bytes_with(e, (uint64_t)(uintptr_t)d_src) > G || decoded + e.size > RANGE_PASS_DECODED)) break;
      U.add(e, (uint64_t)(uintptr_t)d_src);
      max_level = std::max(max_level, e.level); decoded += e.size; t1++;
    }
    st.passes++; st.up += U.bytes;
    const uint64_t up_n = U.bytes;
    HostBuf staged;                                                // (declared in front of the share: given back once its stream has drained)
    DecJob J; DecShare S;
    S.s = std::move(keep);
    J.n = (size_t)up_n; J.mode = 0; J.batch = true; J.given = true; J.timing = false;
    J.tt_stride = 100000u * max_level;
    S.device = dev; S.lo = 0; S.hi = up_n; S.up_lo = 0; S.up_hi = up_n;
    std::vector<uint32_t> cand_of(t1 - t0, ~0u);                  // touched block t0 + i's candidate (~0: its magic is not there)
    if (in) {                                                      // host form: the runs staged in one buffer, the magics checked here
      staged = HostBuf((size_t)up_n);
      if (!staged) return CJS_E_OUT_OF_MEMORY;
      for (const RangeRun& r : U.runs) memcpy(staged.p + r.at, in + r.lo, (size_t)(r.hi - r.lo));
      J.in = staged.p;
      for (size_t i = 0; i < t1 - t0; i++) {
        const uint64_t bp = ix->e[touched[t0 + i]].bitpos;
        uint64_t w = 0;
        for (int q = 0; q < 7; q++) w = (w << 8) | in[(bp >> 3) + q];      // (end_bit > bitpos + 80 and end_bit <= 8 n: inside the stream)
        if (((w >> (8 - (bp & 7))) & 0xFFFFFFFFFFFFull) != MAGIC_BLOCK) continue;
        cand_of[i] = (uint32_t)S.cands.size();
        S.cands.push_back(Cand{U.bit[i], 0u, 0u});
      }
    } else {                                                       // device form: one gather launch, one magic-check launch
      for (size_t i = 0; i < t1 - t0; i++) { cand_of[i] = (uint32_t)i; S.cands.push_back(Cand{U.bit[i], 0u, 0u}); }
      J.upload = [&U, d_src](DecShare* s, uint8_t* dst) {
        std::vector<Slice> sl;
        for (const RangeRun& r : U.runs) range_slices(sl, (uint64_t)(uintptr_t)d_src + r.lo, (uint64_t)(uintptr_t)dst + r.at, r.hi - r.lo);
        Slice* d_sl = nullptr;
        CJS_TRY(s->take((void**)&d_sl, sizeof(Slice) * sl.size()));      // (stays with the share: the copy below may still read `sl` -- it is synchronous for pageable memory)
        if (hipMemcpy(d_sl, sl.data(), sizeof(Slice) * sl.size(), hipMemcpyHostToDevice) != hipSuccess) return (int)CJS_E_HIP;
        s->h2d += sizeof(Slice) * sl.size();
        launch_slices(s->s, d_sl, sl.size());
        return hipGetLastError() != hipSuccess ? (int)CJS_E_HIP : 0;
      };
      J.vet = [&cand_of](DecShare* s) {
        const uint32_t nc = (uint32_t)s->cands.size();
        std::vector<uint64_t> bits(nc); std::vector<uint32_t> ok(nc);
        for (uint32_t c = 0; c < nc; c++) bits[c] = s->cands[c].bit;
        uint64_t* d_bits = nullptr; uint32_t* d_ok = nullptr;
        ShareScratch q(s);
        CJS_TRY(q.take((void**)&d_bits, 8 * (size_t)nc));
        CJS_TRY(q.take((void**)&d_ok, 4 * (size_t)nc));
        if (hipMemcpy(d_bits, bits.data(), 8 * (size_t)nc, hipMemcpyHostToDevice) != hipSuccess) return (int)CJS_E_HIP;
        launch_cand_magic(s->s, s->d_in, s->up_hi, d_bits, nc, d_ok);
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(ok.data(), d_ok, 4 * (size_t)nc, hipMemcpyDeviceToHost, s->s) != hipSuccess ||
            hipStreamSynchronize(s->s) != hipSuccess) return (int)CJS_E_HIP;
        s->h2d += 8 * (size_t)nc; s->d2h += 4 * (size_t)nc;
        std::vector<Cand> kept;                                      // (candidate c is touched block t0 + c until here)
        for (uint32_t c = 0; c < nc; c++) {
          cand_of[c] = ok[c] ? (uint32_t)kept.size() : ~0u;
          if (ok[c]) kept.push_back(s->cands[c]);
        }
        s->cands.swap(kept);
        q.done();
        return 0;
      };
    }
    if (!S.cands.empty()) {
      guarded(S.rc, [&] { dec_phase_a(&J, &S); });
      if (S.rc) return S.rc;
    }
    hipStream_t s = S.s;

    // ---- the blocks that agree with their entries so far become the chain of phases B and C
    std::vector<uint32_t> chain_blk;
    for (size_t i = 0; i < t1 - t0; i++) {
      const uint32_t b = touched[t0 + i], c = cand_of[i];
      const cjs_bz_index_entry& e = ix->e[b];
      V.verdict[b] = RG_MISMATCH;
      if (c == ~0u || S.cands[c].kind != 0) continue;
      const BlockOut& bo = S.bos[c];
      const int v = bz_block_verdict(bo, 100000u * e.level, e.bitpos, false);
      clear_detail();
      if (v || !bo.count || bo.end_bit - (U.bit[i] - e.bitpos) != e.end_bit || bo.crc != e.crc) continue;
      J.chain.push_back(ib_block(bo, S.tt_ptr[c])); chain_blk.push_back(b);
    }
    // ---- a decoded batch: the verdicts of its blocks, then the consumer
    auto use = [&](size_t g0, size_t g1, uint8_t* d_exp, ShareScratch& q) {
      for (size_t k = g0; k < g1; k++) {
        const uint32_t b = chain_blk[k];
        if (J.chain[k].out_len != ix->e[b].size) continue;
        if (J.crc_got[k] != J.chain[k].crc) { V.verdict[b] = RG_BAD_CRC; V.crc_got[b] = J.crc_got[k]; continue; }
        V.verdict[b] = RG_GOOD;
      }
      return consume(RangeBatch{J, S, chain_blk, V, g0, g1, d_exp, q, s});
    };
    CJS_TRY(dec_scratch_batches(J, S, use));
    st.h2d += S.h2d; st.d2h += S.d2h; st.a_batches += S.a_batches; st.b_batches += S.b_batches;
    S.release_keep_stream(keep);
    t0 = t1;
  }
  return 0;
}

void cjs::RangeVerdicts::set_bad_detail(const cjs_bz_index* ix, size_t bad) const {
  char d[96];
  if (verdict[bad] == RG_BAD_CRC) { bad_crc_detail(d, sizeof d, crc_got[bad], ix->e[bad].crc); set_detail("%s", d); }
  else set_detail("index does not match the stream at block %zu", bad);
}

int cjs::check_index_stream(const void* in, size_t n, const cjs_bz_index* idx) {
  if (!in && n) return CJS_E_INVALID_ARG;
  if (idx->stream_bytes != n) { set_detail("the index is of a stream of %llu bytes", (unsigned long long)idx->stream_bytes); return CJS_E_INVALID_ARG; }
  return 0;
}

int cjs::count_then_emit(hipStream_t s, uint64_t nt, uint32_t trail, const std::function<int(uint64_t* cnt)>& count_scan,
                         const std::function<void(const uint64_t* cnt, uint4* out, uint64_t keep)>& emit, void* host_out, uint64_t room, ScanStats& st, uint64_t* res) {
  if (!nt) return drained(s, 0);
  if (nt > 0x7FFFFFFFull) return drained(s, CJS_E_UNSUPPORTED);
  DevBuf d_cnt(8 * (size_t)(nt + trail));
  if (!d_cnt.p) return drained(s, CJS_E_OUT_OF_MEMORY);
  uint64_t* cnt = (uint64_t*)d_cnt.p;
  // from here on no way out without a synchronize: the copies may still be reading the caller's vectors or writing `res`
  int rc = count_scan(cnt);
  if (!rc && (hipGetLastError() != hipSuccess || hipMemcpyAsync(res, cnt + nt, 8 * (size_t)trail, hipMemcpyDeviceToHost, s) != hipSuccess)) rc = CJS_E_HIP;
  if ((rc = drained(s, rc))) return rc;
  st.d2h += 8 * (uint64_t)trail; st.tiles += nt;
  const uint64_t keep = std::min(res[0], room);
  if (!keep) return 0;                                             // (a count query and a batch without a hit: one kernel pass less)
  DevBuf d_out(16 * (size_t)keep);
  if (!d_out.p) return CJS_E_OUT_OF_MEMORY;
  emit(cnt, (uint4*)d_out.p, keep);
  if (hipGetLastError() != hipSuccess || hipMemcpyAsync(host_out, d_out.p, 16 * (size_t)keep, hipMemcpyDeviceToHost, s) != hipSuccess) rc = CJS_E_HIP;
  if ((rc = drained(s, rc))) return rc;
  st.d2h += 16 * keep;
  return 0;
}

namespace {

// The range reads' consumer of the engine: the good blocks' pieces as runs of the scratch (neighbours in both the scratch and the
// layout merged), gathered to their place.  host_out: the host form's buffer in the plan's layout; else d_out.
int range_run(const uint8_t* in, const uint8_t* d_src, const cjs_bz_index* ix, const RangePlan& P, uint8_t* host_out, uint8_t* d_out, RangeVerdicts& V, int dev,
              RangeStats& st) {
  size_t piece_at = 0;                                             // pieces in front of it belong to earlier blocks
  auto deliver = [&](const RangeBatch& B) {
    uint8_t* const d_exp = B.d_exp; hipStream_t s = B.s; ShareScratch& q = B.q;
    struct Run { uint64_t src, to, len; };                        // len bytes from byte src of d_exp to byte `to` of the layout
    std::vector<Run> runs;
    uint64_t packed = 0;
    for (size_t k = B.g0; k < B.g1; k++) {
      const uint32_t b = B.blk[k];
      while (piece_at < P.pieces.size() && P.pieces[piece_at].block < b) piece_at++;
      if (!V.good(b)) continue;
      for (; piece_at < P.pieces.size() && P.pieces[piece_at].block == b; piece_at++) {
        const RangePiece& p = P.pieces[piece_at];
        const uint64_t src = B.J.out_off[k] + p.in_off;
        if (!runs.empty() && runs.back().src + runs.back().len == src && runs.back().to + runs.back().len == p.out) runs.back().len += p.len;
        else runs.push_back(Run{src, p.out, p.len});
        packed += p.len;
      }
    }
    // Host form, a few long runs (one long range, the whole stream): each goes from the scratch straight to its place, no
    // gather.  Else the slice gather: into d_out, or into a packed buffer that goes to the host in one copy.
    const bool direct = host_out && runs.size() <= 16;
    std::vector<Slice> sl;
    uint8_t* d_pack = nullptr; Slice* d_sl = nullptr;
    HostBuf bounce;
    int rc = 0;
    if (!direct && packed) {
      if (host_out) CJS_TRY(q.take((void**)&d_pack, (size_t)packed + 64));
      if (host_out && !(bounce = HostBuf((size_t)packed))) return (int)CJS_E_OUT_OF_MEMORY;
      uint64_t at = 0;
      for (const Run& r : runs) {
        range_slices(sl, (uint64_t)(uintptr_t)(d_exp + r.src), (uint64_t)(uintptr_t)(host_out ? d_pack + at : d_out + r.to), r.len);
        at += r.len;
      }
      CJS_TRY(q.take((void**)&d_sl, sizeof(Slice) * sl.size()));
      // from here on no way out without the synchronize below: the copy may still be reading `sl`
      if (hipMemcpyAsync(d_sl, sl.data(), sizeof(Slice) * sl.size(), hipMemcpyHostToDevice, s) != hipSuccess) rc = CJS_E_HIP;
      else {
        B.S.h2d += sizeof(Slice) * sl.size(); st.slices += sl.size();
        launch_slices(s, d_sl, sl.size());
        if (hipGetLastError() != hipSuccess) rc = CJS_E_HIP;
      }
    }
    if (!rc && host_out && packed) {
      if (direct) { for (const Run& r : runs) if (hipMemcpyAsync(host_out + r.to, d_exp + r.src, (size_t)r.len, hipMemcpyDeviceToHost, s) != hipSuccess) { rc = CJS_E_HIP; break; } }
      else if (hipMemcpyAsync(bounce.p, d_pack, (size_t)packed, hipMemcpyDeviceToHost, s) != hipSuccess) rc = CJS_E_HIP;
      B.S.d2h += packed;
    }
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = CJS_E_HIP;
    if (rc) return rc;
    if (bounce) { uint64_t at = 0; for (const Run& r : runs) { memcpy(host_out + r.to, bounce.p + at, (size_t)r.len); at += r.len; } }
    return 0;
  };
  return range_engine(in, d_src, ix, P.touched, V, dev, st, deliver);
}

// The verdict of every range from the verdicts of the blocks: status, and the detail of the lowest-index failing range's first bad
// block.  `fail` gets 1 for a failing range.
void range_verdicts(const cjs_bz_index* ix, const RangePlan& P, const uint64_t* off, size_t count, const RangeVerdicts& V, int32_t* status, std::vector<uint8_t>& fail) {
  const size_t nblk = ix->e.size();
  std::vector<size_t> next_bad(nblk + 1, nblk);                    // the first bad block at or behind b
  for (size_t b = nblk; b-- > 0;) next_bad[b] = !V.good(b) ? b : next_bad[b + 1];
  fail.assign(count, 0);
  bool first = true;
  for (size_t k = 0; k < count; k++) {
    status[k] = 0;
    if (!P.lay_len[k]) continue;
    const size_t b0 = range_block_of(ix, off[k]), b1 = range_block_of(ix, off[k] + P.lay_len[k] - 1), bad = next_bad[b0];
    if (bad > b1) continue;
    status[k] = CJS_E_DATA_ERROR; fail[k] = 1;
    if (first) V.set_bad_detail(ix, bad);
    first = false;
  }
}

}  // namespace

// The range reads' core with the result on the device (range_engine.h), for a caller that has checked its arguments.
int cjs::range_read_to_device(const uint8_t* in, const uint8_t* d_src, const cjs_bz_index* ix, const uint64_t* off, const uint64_t* len, size_t count,
                              uint8_t* d_out, RangeVerdicts& V, int dev, RangeStats& st) {
  RangePlan P;
  CJS_TRY(range_plan(ix, off, len, count, P));
  if (P.touched.empty()) return 0;
  return range_run(in, d_src, ix, P, nullptr, d_out, V, dev, st);
}

namespace {

int range_check_args(const void* in, size_t n, const cjs_bz_index* idx, const uint64_t* off, const uint64_t* len, size_t count, const size_t* out_off,
                     const size_t* out_len, const int32_t* status) {
  if (!idx || (count && (!off || !len || !out_off || !out_len || !status))) return CJS_E_INVALID_ARG;
  return check_index_stream(in, n, idx);
}

void range_debug(const char* form, const cjs_bz_index* ix, const RangePlan& P, size_t count, const RangeStats& st) {
  if (!env_debug()) return;
  fprintf(stderr, "[cjs range] %s: %zu ranges, %llu bytes, %zu of %zu blocks touched, %u passes (%u row batches, %u inverse-BWT batches), upload %llu B, %zu slices, H2D %llu D2H %llu\n",
          form, count, (unsigned long long)P.total, P.touched.size(), ix->e.size(), st.passes, st.a_batches, st.b_batches, (unsigned long long)st.up, st.slices,
          (unsigned long long)st.h2d, (unsigned long long)st.d2h);
}

}  // namespace

extern "C" int cjs_bzip2_index_build(const uint8_t* in, size_t n, int multistream, cjs_bz_index** idx, const cjs_opts* opts) {
  if (!idx) return CJS_E_INVALID_ARG;
  *idx = nullptr;
  CJS_GUARD_BEGIN
  long nbk = 0;
  std::vector<cjs_bz_index_entry> e;
  CJS_TRY(bunzip_core(in, n, multistream, 1, 0, nullptr, nullptr, nullptr, nullptr, 0, &nbk, opts, &e));
  e.resize((size_t)nbk);
  return bz_index_make(e.data(), e.size(), n, multistream != 0, idx);
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

extern "C" int cjs_bzip2_read_ranges(const uint8_t* in, size_t n, const cjs_bz_index* idx, const uint64_t* off, const uint64_t* len, size_t count,
                                     uint8_t** out, size_t* out_off, size_t* out_len, int32_t* status, const cjs_opts* opts) {
  if (!out) return CJS_E_INVALID_ARG;
  *out = nullptr;
  clear_detail();
  CJS_GUARD_BEGIN
  CJS_TRY(range_check_args(in, n, idx, off, len, count, out_off, out_len, status));
  RangePlan P;
  CJS_TRY(range_plan(idx, off, len, count, P));
  HostBuf host((size_t)std::max<uint64_t>(P.total, 1));          // (given back on every failing path)
  if (!host) return CJS_E_OUT_OF_MEMORY;
  RangeVerdicts V(idx); std::vector<uint8_t> fail;
  RangeStats st;
  if (!P.touched.empty()) {
    CallDevice cd;
    CJS_TRY(cd.select(opts));
    CJS_TRY(range_run(in, nullptr, idx, P, host.p, nullptr, V, cd.dev, st));
  }
  range_verdicts(idx, P, off, count, V, status, fail);
  size_t at = 0;                                                   // the layout behind the verdicts: a failed range takes no room
  for (size_t k = 0; k < count; k++) {
    out_off[k] = at; out_len[k] = fail[k] ? 0 : (size_t)P.lay_len[k];
    if (out_len[k] && at != P.lay_off[k]) memmove(host.p + at, host.p + P.lay_off[k], out_len[k]);
    at += out_len[k];
  }
  range_debug("host", idx, P, count, st);
  *out = host.release();
  return 0;
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

extern "C" int cjs_bzip2_read_ranges_device(const uint8_t* d_in, size_t n, const cjs_bz_index* idx, const uint64_t* off, const uint64_t* len, size_t count,
                                            uint8_t* d_out, size_t out_cap, size_t* out_off, size_t* out_len, int32_t* status, size_t* out_need,
                                            const cjs_opts* opts) {
  if (!out_need || (!d_out && out_cap)) return CJS_E_INVALID_ARG;
  *out_need = 0;
  clear_detail();
  CJS_GUARD_BEGIN
  CJS_TRY(range_check_args(d_in, n, idx, off, len, count, out_off, out_len, status));
  RangePlan P;
  CJS_TRY(range_plan(idx, off, len, count, P));
  *out_need = (size_t)P.total;
  for (size_t k = 0; k < count; k++) { out_off[k] = (size_t)P.lay_off[k]; out_len[k] = (size_t)P.lay_len[k]; status[k] = 0; }
  if (P.total > out_cap) return CJS_E_OUTPUT_TOO_SMALL;           // (known from the index alone: nothing is launched, d_out untouched)
  if (P.touched.empty()) return 0;
  CallDevice cd;
  CJS_TRY(cd.select(opts));
  if (!on_device(d_in, cd.dev) || !on_device(d_out, cd.dev)) return CJS_E_INVALID_ARG;      // (no host pointer reaches a kernel)
  RangeVerdicts V(idx); std::vector<uint8_t> fail;
  RangeStats st;
  CJS_TRY(range_run(nullptr, d_in, idx, P, nullptr, d_out, V, cd.dev, st));
  range_verdicts(idx, P, off, count, V, status, fail);
  for (size_t k = 0; k < count; k++) if (fail[k]) out_len[k] = 0;      // (the region keeps its place)
  range_debug("device", idx, P, count, st);
  return 0;
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}
