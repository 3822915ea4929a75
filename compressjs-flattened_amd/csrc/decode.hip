// decode.hip — Bzip2.decompressFile (Bunzip.decode, J/Bzip2_joined_.js:1769-1796) on the MI355X: the map of the decoder, the
// helpers every driver shares (header, level, block verdict, output offsets) and the single-stream driver.  The engine
// (dec_engine.h) runs the steps below in three phases, each a file of its kernels and its host steps: dec_blocks.hip (phase A:
// 1 and 2), dec_ibwt.hip (phase B: 4, and the lengths of 5), dec_unrle1.hip (phase C: 5 and 6); dec_plan.h holds their host
// arithmetic.  The other drivers have files of their own: dec_batch.hip (host batch, device-resident single and batch),
// dec_recover.hip, range.hip, dec_stream.hip.
//
// The reference decodes block after block from one bit cursor.  Blocks carry no length field, so here:
//   1. bz_magic_scan     every bit offset of the stream is tested against the 48-bit block / end-of-stream
//                        magics (:1434-1439) -> candidate list (a few hundred entries);
//   2. bz_decode_block   one wave per candidate: header, selector list, code-length tables, then the
//                        bit-serial Huffman + RUNA/RUNB + MTF decode (:1456-1670) on lane 0 with
//                        10-bit direct lookup tables built by the whole wave from the reference's
//                        limit/base/permute semantics; yields the BWT bytes, their histogram, the end bit;
//   3. host              walks the chain 32 -> end(block0) -> end(block1) ... over the candidates (a false
//                        2^-48 candidate inside payload bits is simply never reached), folds CRCs;
//   4. inverse BWT       T vector by a stable radix pass keyed (block, byte) (:1677-1690), then the LF walk
//                        (:1732-1737) — n dependent gathers — made k-way parallel by splitter list ranking:
//                        every 128th slot is a splitter, lanes walk to the next splitter, one workgroup per block
//                        ranks the splitters (pointer jumping in LDS), lanes re-walk writing bytes at their final offsets;
//   5. RLE1 expansion    (:1738-1753) parsed in parallel: a count byte follows 4 equal literals; inside a
//                        stretch of equal bytes the literal/count phase has period 5 and the only carried
//                        state (does the stretch start with a count byte?) is a 2-state function scan;
//   6. CRC check         per block over the output bytes (crc.hip's slice + GF(2) combine), :1756-1761.
// Recovery of damaged data (dec_recover.hip: cjs_bzip2_recover, no reference equivalent: the job of bzip2recover) is 1, 2 and 4-6
// over EVERY decodable candidate, with step 3 replaced by a selection of the intact, non-overlapping ones; an indexed range read
// (range.hip) is 2 and 4-6 over the blocks its index names.
#include "dec_engine.h"
#include <stdlib.h>
#include <string.h>

using namespace cjs;

// ---------------------------------------------------------------- host driver
// mode 0: Bunzip.decode (:1769-1796); mode 1: Bunzip.table (:1823-1863) -> (bit position, size) per block, no bytes;
// mode 2: Bunzip.decodeBlock (:1797-1818) -> the single block whose magic starts at `at_bit`.
//
// The job is cut into per-device shares (SURVEY §8e "Bzip2 decompress"; cjs_opts.n_devices / CJS_DEVICES, one host thread
// per share; several shares may sit on one GPU):
//   A  per share   upload its byte range (+ one worst-case block of overlap), magic scan, speculative decode of every
//                  candidate that STARTS in the share
//   -  host        chain walk 32 -> end(block 0) -> end(block 1) ... over all shares' candidates: stream CRC fold,
//                  multistream restarts (each stream keeps its own level, :1787-1792)
//   B  per share   inverse BWT of the chain blocks it decoded, in batches (bounded scratch), RLE1 length pass
//   -  host        exclusive prefix sum of the decoded lengths -> output offsets
//   C  per share   RLE1 expansion + block CRCs per batch, D2H straight to the final offsets
// No data moves between devices; the exchanged quantities are (end bit, count, crc) per candidate and a length per block.
//
// The phases: dec_blocks.hip (A), dec_ibwt.hip (B), dec_unrle1.hip (C), each a short list of named steps over its own kernels.
// Eight drivers sit on them, through dec_engine.h (the arena, the share, the job, the walk and the glue between the phases):
//   here             bunzip_core (single stream, shares over devices; cjs_bzip2_decompress, _decompress_block, _table, and the
//                    table pass of cjs_bzip2_index_build)
//   dec_batch.hip    dec_batch_group (host batch), dev_single_* (device-resident single stream), dev_group_* (device-resident batch)
//   dec_recover.hip  recover_core (recovery, both forms)
//   range.hip        range_run (indexed range reads, both forms)
//   dec_stream.hip   dec_step (streaming)
// A driver holds what is particular to it: where the bytes come from and where they go.
namespace cjs {

double ms_since(std::chrono::steady_clock::time_point a) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count(); }

// _start_bunzip (:1408-1427) on the first four bytes h of an input (or of a member stream) of n bytes: 0 and the level, or
// CJS_E_NOT_BZIP_DATA and the detail text in *why (the caller sets it, or stores it with its input)
int bz_header_check(const uint8_t* h, size_t n, int* level, const char** why) {
  if (n < 4 || h[0] != 'B' || h[1] != 'Z' || h[2] != 'h') { *why = "bad magic"; return CJS_E_NOT_BZIP_DATA; }
  *level = h[3] - '0';
  if (*level < 1 || *level > 9) { *why = "level out of range"; return CJS_E_NOT_BZIP_DATA; }
  return 0;
}

// The scratch rows are sized for the largest level any member stream can have: a multistream file may change level
// between members (:1787-1792), so every byte-aligned "BZh<d>" followed by a block or end-of-stream magic counts.
int bz_max_level(const uint8_t* in, size_t n, int level, bool multistream) {
  int max_level = level;
  if (multistream) {
    for (const uint8_t* p = in + 4; p + 10 <= in + n && (p = (const uint8_t*)memchr(p, 'B', (size_t)(in + n - 9 - p))) != nullptr; p++) {
      if (p[1] != 'Z' || p[2] != 'h' || p[3] < '1' || p[3] > '9') continue;
      uint64_t m = 0; for (int i = 0; i < 6; i++) m = (m << 8) | p[4 + i];
      if ((m == MAGIC_BLOCK || m == MAGIC_END) && p[3] - '0' > max_level) max_level = p[3] - '0';
    }
  }
  return max_level;
}

// A decoded block candidate as the walk meets it (:1440-1450, 1647, 1663): 0 if it joins the chain, else the error.
int bz_block_verdict(const BlockOut& bo, uint32_t dbuf_size, uint64_t bitpos, bool timing) {
  if (timing) fprintf(stderr, "[cjs dec] block at bit %llu: err %d count %u orig %u crc %08x end %llu\n", (unsigned long long)bitpos, bo.err, bo.count, bo.orig, bo.crc, (unsigned long long)bo.end_bit);
  if (bo.err != CJS_E_OBSOLETE_INPUT && bo.orig > dbuf_size) { set_detail("initial position out of bounds"); return CJS_E_DATA_ERROR; }   // :1449-1450
  if (bo.err) return bo.err;
  if (bo.count > dbuf_size) return CJS_E_DATA_ERROR;             // decoded with the largest level's limit: this stream's is lower (:1647,1663)
  return 0;
}

// exclusive prefix sum of the chain's decoded lengths (phase B's) -> J.out_off; returns the total
uint64_t chain_out_offsets(DecJob& J) {
  const size_t nb = J.chain.size();
  J.out_off.assign(nb + 1, 0);
  for (size_t k = 0; k < nb; k++) J.out_off[k + 1] = J.out_off[k] + J.chain[k].out_len;
  return J.out_off[nb];
}

// ---------------------------------------------------------------- the single-stream driver
int bunzip_core(const uint8_t* in, size_t n, int multistream, int mode, uint64_t at_bit, uint8_t** out, size_t* out_n,
                uint64_t* tab_pos, uint32_t* tab_size, long tab_cap, long* tab_n, const cjs_opts* opts,
                std::vector<cjs_bz_index_entry>* tab_ix) {      // (mode 1: an index entry per block as well)
  if (out) *out = nullptr;
  if (out_n) *out_n = 0;
  if (tab_n) *tab_n = 0;
  clear_detail();
  CJS_TRY(select_device(opts));
  int level = 0; const char* why = nullptr;
  if (bz_header_check(in, n, &level, &why)) { set_detail("%s", why); return CJS_E_NOT_BZIP_DATA; }
  int ndev = 0, dev0 = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || hipGetDevice(&dev0) != hipSuccess) return CJS_E_NO_DEVICE;

  DecJob J; J.in = in; J.n = n; J.mode = mode;
  J.timing = env_debug();
  J.tt_stride = 100000u * (uint32_t)bz_max_level(in, n, level, multistream && mode != 2);

  // shares: contiguous byte ranges, one per requested device slot
  uint32_t nsh = Opts(opts).n_devices;
  if (nsh < 1 || mode == 2) nsh = 1;
  if (nsh > 64) nsh = 64;
  if ((size_t)nsh * 65536 > n) nsh = (uint32_t)(n / 65536 ? n / 65536 : 1);     // tiny inputs: one share
  const uint64_t overlap = dec_extent(J.tt_stride);
  RestoreDevice restore{dev0};                                                  // after the shares have been released
  HostBuf host;                                                                 // (in front of the shares: given back once their streams have drained)
  std::vector<DecShare> sh(nsh);
  for (uint32_t i = 0; i < nsh; i++) {
    DecShare& S = sh[i];
    S.device = nsh == 1 ? dev0 : (int)(i % (uint32_t)ndev);
    S.lo = (uint64_t)n * i / nsh; S.hi = (uint64_t)n * (i + 1) / nsh;
    S.up_lo = S.lo & ~(uint64_t)255;
    S.up_hi = std::min<uint64_t>(n, S.hi + overlap);
  }
  if (mode == 2) {                                                             // one block: upload from its byte on
    sh[0].lo = std::min<uint64_t>(at_bit >> 3, n); sh[0].hi = std::min<uint64_t>(n, sh[0].lo + 1);
    sh[0].up_lo = sh[0].lo & ~(uint64_t)255; sh[0].up_hi = std::min<uint64_t>(n, sh[0].hi + overlap);
  }
  const auto T0 = std::chrono::steady_clock::now();
  int rc = for_each_share(sh, &J, dec_phase_a);
  if (rc) return rc;
  const double ms_a = ms_since(T0);

  // ---- chain walk over all shares' candidates (Bunzip.decode :1776-1794)
  const WalkCands C(sh.data(), nsh);
  std::vector<uint32_t> chain_share;
  WalkState wst;                                                 // (a whole walk from the header on; met reads the member's level of it)
  auto met = [&](long ci, uint64_t pos) {
    if (C.kind(ci) != 0) return;
    J.chain_bits.push_back(pos); chain_share.push_back(C.share[(size_t)ci]);
    if (tab_ix) tab_ix->push_back(cjs_bz_index_entry{pos, C.bo(ci).end_bit, 0u, C.bo(ci).crc, wst.dbuf_size / 100000u, 0u});
  };
  if (mode == 2) {                                               // reader.seekBit(pos); _get_next_block() (:1803-1805)
    const long ci = C.find(at_bit);
    if (ci < 0) rc = CJS_E_NOT_BZIP_DATA;
    else if (C.kind(ci) == 0) {
      rc = bz_block_verdict(C.bo(ci), 100000u * (uint32_t)level, at_bit, J.timing);
      if (!rc) { J.chain.push_back(C.chain_block(ci)); met(ci, at_bit); }
    }
  } else rc = walk_chain(J, C, in, n, multistream, mode, met, &wst);
  // The reference decodes block after block and checks every block's CRC before it reads on (:1756-1761), so an error met
  // by the walk (bad stream CRC, damaged later block, broken chain) is reported only if every block in front of it
  // passes its own CRC check: keep it pending and run the rest of the pipeline, without output, over the chain so far.
  const int pending_rc = rc;
  char pending_detail[192];
  snprintf(pending_detail, sizeof pending_detail, "%s", cjs_last_error_detail());
  clear_detail();
  rc = 0;
  const size_t nb = J.chain.size();
  if (nb == 0) {
    if (pending_rc) { set_detail("%s", pending_detail); return pending_rc; }
    if (out) { *out = (uint8_t*)malloc(1); if (!*out) return CJS_E_OUT_OF_MEMORY; }
    return 0;
  }
  {  // the chain is increasing in bit position, so every share owns one contiguous run of it
    size_t k = 0;
    for (uint32_t i = 0; i < nsh; i++) { sh[i].c0 = k; while (k < nb && chain_share[k] == i) k++; sh[i].c1 = k; }
    if (k != nb) return CJS_E_DATA_ERROR;      // a chain that runs backwards: corrupt input
  }
  const auto T1 = std::chrono::steady_clock::now();
  rc = for_each_share(sh, &J, dec_phase_b);
  if (rc) return rc;
  const double ms_b = ms_since(T1);
  const uint64_t total = chain_out_offsets(J);
  if (out && !pending_rc) { host = HostBuf(total ? (size_t)total : 1); if (!(J.host = host.p)) return CJS_E_OUT_OF_MEMORY; }
  const auto T2 = std::chrono::steady_clock::now();
  rc = for_each_share(sh, &J, dec_phase_c);
  const double ms_c = ms_since(T2);
  for (auto& x : sh) x.release();                              // (the streams have drained before J.host can go back)
  if (J.timing) {
    fprintf(stderr, "[cjs dec] %u share(s): upload + magic scan + block decode %.2f ms, inverse BWT + RLE1 lengths %.2f ms, RLE1 + CRC + D2H %.2f ms\n", nsh, ms_a, ms_b, ms_c);
    for (uint32_t i = 0; i < nsh; i++) fprintf(stderr, "[cjs dec]   share %u (device %d): %zu candidates, blocks [%zu, %zu): %.2f / %.2f / %.2f ms\n", i, sh[i].device,
                                               sh[i].cands.size(), sh[i].c0, sh[i].c1, sh[i].ms_a, sh[i].ms_b, sh[i].ms_c);
  }
  if (rc) return rc;
  if (pending_rc) { set_detail("%s", pending_detail); return pending_rc; }
  if (tab_n) {
    *tab_n = (long)nb;
    for (size_t k = 0; k < nb && (long)k < tab_cap; k++) { tab_pos[k] = J.chain_bits[k]; tab_size[k] = J.chain[k].out_len; }
    if (tab_ix) for (size_t k = 0; k < nb; k++) (*tab_ix)[k].size = J.chain[k].out_len;
  }
  if (out) { *out = host.release(); *out_n = (size_t)total; }
  return 0;
}

}  // namespace cjs

extern "C" int cjs_bzip2_decompress(const uint8_t* in, size_t n, int multistream, uint8_t** out, size_t* out_n, const cjs_opts* opts) {
  if (!out || !out_n) return CJS_E_INVALID_ARG;
  CJS_GUARD_BEGIN
  return bunzip_core(in, n, multistream, 0, 0, out, out_n, nullptr, nullptr, 0, nullptr, opts);
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}
extern "C" int cjs_bzip2_decompress_block(const uint8_t* in, size_t n, uint64_t bitpos, uint8_t** out, size_t* out_n, const cjs_opts* opts) {
  if (!out || !out_n) return CJS_E_INVALID_ARG;
  CJS_GUARD_BEGIN
  return bunzip_core(in, n, 0, 2, bitpos, out, out_n, nullptr, nullptr, 0, nullptr, opts);
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}
extern "C" long cjs_bzip2_table(const uint8_t* in, size_t n, int multistream, uint64_t* bitpos, uint32_t* size, long cap, const cjs_opts* opts) {
  CJS_GUARD_BEGIN
  long nbk = 0;
  const int rc = bunzip_core(in, n, multistream, 1, 0, nullptr, nullptr, bitpos, size, cap, &nbk, opts);
  return rc ? (long)rc : nbk;
  CJS_GUARD_END((long)CJS_E_OUT_OF_MEMORY, (long)CJS_E_HIP)
}
