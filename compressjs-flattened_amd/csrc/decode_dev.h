// decode_dev.h -- device-side pieces of Bzip2 decode shared by dec_blocks.hip (the single-stream kernels) and batch_dec.hip (their
// batch forms): candidate and block records, the bit readers, the code tables and the chain helpers of stage 2; the RLE1 tile
// state that dec_ibwt.hip sizes and dec_unrle1.hip fills; and the launch functions of batch_dec.hip and dec_device.hip.  The host
// side of the engine is dec_engine.h.
#pragma once
#include "bz_frame.h"
#include "cjs_internal.h"
#include "dec_plan.h"
#include "prims.hpp"

namespace cjs {

// (MAGIC_BLOCK, MAGIC_END: bz_frame.h; SPL, the splitter spacing of the inverse BWT; GROUP_SYMS, MAX_SELECTORS: dec_plan.h)

struct Cand { uint64_t bit; uint32_t kind; uint32_t pad; };      // kind 0 = block, 1 = end of stream; pad = row of the block candidate in the decode buffer (set by the host)
struct BlockOut {
  uint64_t end_bit;       // first bit after the block's EOB code
  uint32_t count;         // decoded BWT bytes (dbufCount)
  uint32_t orig;          // origPointer
  uint32_t crc;           // stored block CRC
  int32_t err;            // 0 or a CJS_E_* code
};

// ---------------------------------------------------------------- 2. block decode (one wave per candidate)
struct BitReader {
  const uint8_t* p; uint64_t nbits, pos;
  uint64_t win; uint64_t wbyte;                                      // cached big-endian window of bytes [wbyte, wbyte+8)
  __device__ __forceinline__ void refill() {
    wbyte = pos >> 3;
    const uint64_t nbytes = (nbits + 7) >> 3;
    uint64_t w = 0;
    if (wbyte + 8 <= nbytes) {
#pragma unroll
      for (int i = 0; i < 8; i++) w = (w << 8) | p[wbyte + i];
    } else {
#pragma unroll
      for (int i = 0; i < 8; i++) w = (w << 8) | (wbyte + i < nbytes ? p[wbyte + i] : 0);   // zeros past EOF (:149)
    }
    win = w;
  }
  __device__ __forceinline__ uint32_t peek(int k) {                  // next k <= 25 bits
    uint64_t off = pos - (wbyte << 3);
    if (pos < (wbyte << 3) || off + (uint64_t)k > 64) { refill(); off = pos - (wbyte << 3); }
    return (uint32_t)((win << off) >> (64 - k));
  }
  __device__ __forceinline__ void skip(int k) { pos += k; if (pos > nbits) pos = nbits; }
  __device__ __forceinline__ uint32_t get(int k) { const uint32_t v = peek(k); skip(k); return v; }
};

// Canonical code of one table in first-code form: the codes of length L are first[L] .. first[L] + cnt[L] - 1, handed out in
// symbol order (bysym[start[L] ..]), and first[L + 1] = (first[L] + cnt[L]) << 1.  A prefix j of L bits that is not a code of a
// shorter length satisfies j >= first[L], so "j - first[L] < cnt[L]" decides -- the same decisions as the reference's
// limit / base / permute walk (:1522-1581, :1605-1616) on every length table, complete or not.
struct DecShared {
  uint32_t first[6][22];           // first code of each length
  uint16_t cnt[6][22];             // symbols of each length
  uint16_t start[6][22];           // index of the first symbol of each length in bysym
  uint16_t bysym[6][260];          // symbols ordered by (length, symbol)
  uint8_t minlen[8], maxlen[8];
  uint8_t length[6][260];
  uint8_t sym_to_byte[256];
  // left-justified (20-bit) end of the codes of each length, for the branch-free length rule of bz_chain: the code that starts
  // with the 20 bits x has length 1 + #{L in 1..19 : x >= limp[L]} and exists iff x < limp[20]  (limp[L] = 0 below the shortest
  // length, = (first[L] + cnt[L]) << (20 - L) from there to the longest, then 2^20 up to L = 19; limp[20] = the longest's)
  uint32_t limp[6][21];
};

// big-endian 32-bit word `dw` of the stream, zeros past the end (the reference's reader yields zero bits there, :149)
__device__ __forceinline__ uint32_t load_be32(const uint8_t* in, uint64_t n, uint64_t dw) {
  const uint64_t b = dw * 4;
  if (b + 4 <= n) return __builtin_bswap32(*reinterpret_cast<const uint32_t*>(in + b));       // `in` is a hipMalloc'd copy: 4-byte aligned
  uint32_t v = 0;
  for (int i = 0; i < 4; i++) v = (v << 8) | (b + i < n ? in[b + i] : 0u);
  return v;
}
// 4096-bit register window on the stream: lane j holds words base+j (A) and base+64+j (B); all cursor state is wave-uniform
struct BitWin {
  const uint8_t* in; uint64_t n; uint64_t base; uint32_t A, B;
  __device__ __forceinline__ void init(uint64_t pos, int lane) { base = pos >> 5; A = load_be32(in, n, base + lane); B = load_be32(in, n, base + 64 + lane); }
  __device__ __forceinline__ void ensure(uint64_t pos, int lane) {        // afterwards (pos >> 5) - base < 64
    while ((pos >> 5) - base >= 64) {
      if ((pos >> 5) - base >= 128) { init(pos, lane); return; }
      A = B; base += 64; B = load_be32(in, n, base + 64 + lane);
    }
  }
  __device__ __forceinline__ uint32_t word(uint32_t k) const { return k < 64 ? __builtin_amdgcn_readlane(A, k) : __builtin_amdgcn_readlane(B, k - 64); }
  __device__ __forceinline__ uint32_t peek(uint64_t pos, int k) const {   // k <= 32 bits at pos (uniform), window must cover it
    const uint32_t d = (uint32_t)((pos >> 5) - base);
    const uint64_t w = ((uint64_t)word(d) << 32) | word(d + 1);
    return (uint32_t)((w << (pos & 31)) >> (64 - k));
  }
};

// Block header and code lengths (lane 0, serial), selector list and decode tables (whole wave).  Executed by ONE wave; the results
// are wave-uniform scalars.  Returns 0 or a CJS_E_* code.  `selp`: LDS scratch of 4096 words (the unary values, a nibble each).
// a list of eight nibbles: nibble j to the front / the list x read at the positions y holds
__device__ __forceinline__ uint32_t nib_to_front(uint32_t st, uint32_t j) {
  const uint32_t val = (st >> (4u * j)) & 15u, low = st & ((1u << (4u * j)) - 1u);
  return (st & ~((1u << (4u * j + 4u)) - 1u)) | (low << 4) | val;
}
__device__ __forceinline__ uint32_t nib_compose(uint32_t x, uint32_t y) {
  uint32_t r = 0;
#pragma unroll
  for (int p = 0; p < 8; p++) r |= ((x >> (4u * ((y >> (4 * p)) & 15u))) & 15u) << (4 * p);
  return r;
}
// dec_prologue(): bz_stage2.h (one copy per form of bz_chain, each with a single caller)

// ---------------------------------------------------------------- 2b. block decode in stages
// The Huffman chain of a block looks serial -- the table changes every 50 symbols, so there is no self-synchronisation to exploit
// -- but the only thing one group of 50 symbols hands to the next is WHERE IT ENDS.  So:
//   bz_chain        one workgroup per candidate: header, selector list and code tables (wave 0, in 2048-bit stretches), then up to
//                   four groups per step: for every bit position i of a group's positions thread i looks up the length of the code
//                   that WOULD start there: next[i] = i + len.  Five rounds of pointer doubling in LDS (next^2 .. next^32) give
//                   next^50(0) = 2 + 16 + 32 for the first group; the groups behind it get tables of their own over positions
//                   placed ahead, built in the same rounds (chain_tables).  About ten LDS round trips per 200 symbols instead of
//                   50 x (lookup + hop) per group by one lone wave.
//   bz_group_syms   one lane per group, all groups of all candidates at once: the 50 symbols from the group's start; the first
//                   end-of-block symbol and the first undecodable code of the block by 64-bit atomic minima.
//   bz_sym_ops      one workgroup per candidate over the symbols in front of the end-of-block: RUNA/RUNB digits -> byte counts,
//                   running output offset, every rank symbol leaves as (rank, output offset).  No move-to-front, no output bytes.
//   bz_mtf_tiles    the move-to-front of 256 consecutive rank ops of a block, started from the identity list, by one wave
//                   (list as bytes across the lanes, shift by wave_shr DPP): op j becomes q_j = the slot of the TILE-START
//                   list it reads, and the tile leaves its permutation P_t.   All tiles of all blocks in parallel.
//   bz_mtf_chunk_perm + bz_mtf_compose  chain the tiles: start list L_(t+1)[p] = L_t[P_t[p]] (an LDS gather per tile), in chunks of 64 tiles.
//   bz_mtf_emit     one thread per op: byte = L_t[q_j] at its offset, and the zero-rank run behind it (the gap to the next
//                   op's offset) is filled with the same byte (long runs by the whole wave).
// Same results as the reference loop (:1597-1670): every way it can fail there is DATA_ERROR, so a block is good iff its first
// end-of-block symbol comes before its first undecodable code, the selectors do not run out first, and the bytes fit the block.
struct RowTab {                    // per candidate row, in global memory between the stages
  uint16_t fast[6][1024];          // (sym << 5) | len by the next 10 bits, 0 = not decodable within 10 bits
  uint32_t first[6][22];
  uint16_t cnt[6][22], start[6][22], bysym[6][260];
  uint8_t minlen[8], maxlen[8];
  uint32_t sym_total, group_count, n_sel, err;      // err: the header's verdict
  uint64_t data_bit;               // first bit of the symbol data
  uint32_t crc, orig;
  uint32_t ngroups_ok;             // groups whose start bit is known (the chain's extent)
  uint32_t pad;
  unsigned long long eob_key;      // min over end-of-block symbols of (symbol index << 32 | bit behind the code - data_bit); ~0 = none
  unsigned long long err_key;      // min over undecodable codes of (symbol index << 32); ~0 = none
};
constexpr uint32_t CH_T = 512;                  // threads of bz_chain
constexpr uint32_t CH_SPAN = 1024;              // bit positions of a group's span (50 codes of <= 20 bits)
constexpr uint32_t CH_ARR = CH_SPAN + 64;
constexpr uint32_t CH_NONE = CH_ARR - 1;         // next[] of a position where no code of the table starts (an entry of its own, like the positions behind a span)
constexpr uint32_t CH_WIN = CH_T - 64;          // positions of a table in a step's first attempt: one per thread, the last 64 map to themselves
constexpr uint32_t CH_ARR2 = CH_T + 64;         // the later groups' tables: CH_WIN positions, and 64 + 64 that map to themselves
constexpr uint32_t CH_NONE2 = CH_ARR2 - 1;
constexpr uint32_t CH_WORDS = 2048;             // 32-bit words of the stream kept in LDS (65536 bits: ~180 groups of text)


// bz_chain's tables: level lv (next^(2^lv)) of table t by byte offset.  A level is read by the round behind it only (the hops aside: 1, 4
// and 5), so four arrays hold the six: 0 and 3 share one, 2 and 5 another -- and the step behind writes its level 0 where this step's
// last lookups (level 5) do not read.
__host__ __device__ constexpr int ch_slot(int lv) { return lv == 1 ? 0 : lv == 4 ? 1 : (lv == 2 || lv == 5) ? 2 : 3; }
template <uint32_t N> __device__ __forceinline__ uint32_t ch_ld(uint16_t (*t)[N], int lv, uint32_t off) { return *reinterpret_cast<const uint16_t*>(reinterpret_cast<const char*>(t[ch_slot(lv)]) + off); }
template <uint32_t N> __device__ __forceinline__ void ch_st(uint16_t (*t)[N], int lv, uint32_t i, uint32_t v) { t[ch_slot(lv)][i] = (uint16_t)v; }
// The 20 bits at bit o of the window
__device__ __forceinline__ uint32_t chain_bits(const uint32_t* wbuf, uint32_t o) {
  const uint32_t w0 = wbuf[o >> 5], w1 = wbuf[(o >> 5) + 1];
  return (uint32_t)(((((uint64_t)w0 << 32) | w1) << (o & 31)) >> 44);
}
// The position behind the code that starts at position i with the 20 bits x20 under table g (CH_NONE: no code starts there).  e is the
// entry of the 12-bit direct table: the length of a code of <= 12 bits, CH_NOCODE, or 0 for a longer code, whose length is 13 + the
// number of lengths 13 .. 19 whose left-justified codes all lie below x20 (well under a percent of ARBITRARY bit offsets: one wave in
// four holds one; with a 10-bit table nearly every wave did and paid the compares).
constexpr uint32_t CH_NOCODE = 0xFF;
__device__ __forceinline__ uint32_t chain_next(const DecShared& S, int g, uint32_t e, uint32_t x20, uint32_t i, uint32_t none) {
  if (e) return e == CH_NOCODE ? none : i + e;
  uint32_t len = 13;
#pragma unroll
  for (int l = 13; l <= 19; l++) len += x20 >= S.limp[g][l] ? 1u : 0u;
  return x20 < S.limp[g][20] ? i + len : none;
}
// One step's tables for NT groups (k on A from its known start, k + q on L[q - 1] from bit start[q - 1] of the step): next^1, then five
// rounds of doubling.  Tables hold BYTE OFFSETS (2 x position) into a level's array, and every position behind a table's last (>= 64 of
// them: a code is at most 20 bits) maps to itself, as does CH_NONE: a chain that has left its positions, or met one where no code
// starts, stays where it is without a compare -- a round is one gather and one store per table, all threads on all tables, no branch
// (the CU's scalar unit serves every wave's branches and address arithmetic: with one thread per position and table, and a branch
// around each, those instructions outnumbered the vector ones three to one and set the pace).  e[q]: where group k + q ends, in
// positions of its table (every lane the same value; CH_NONE / CH_NONE2 or beyond the table's positions: not known from this step).
// Group k's 50 codes are 2 + 16 + 32: the first two hops as soon as their table stands, beside the following round's gathers.
struct ChainLater { uint16_t (*t)[CH_ARR2]; int g; uint32_t start; };
template <int NT>
__device__ __forceinline__ void chain_tables(const DecShared& S, const uint8_t (*len12)[4096], const uint32_t* wbuf, uint16_t (*A)[CH_ARR], const ChainLater (&L)[3],
                                             uint32_t i, uint32_t o0, int g, uint32_t span, bool whole, uint32_t (&e)[4]) {
  // (the tables' loads side by side: two LDS latencies for all of them)
  uint32_t x[NT], en[NT], m[NT];
  x[0] = chain_bits(wbuf, o0 + i);
#pragma unroll
  for (int q = 1; q < NT; q++) x[q] = chain_bits(wbuf, o0 + L[q - 1].start + i);
  en[0] = len12[g][x[0] >> 8];
#pragma unroll
  for (int q = 1; q < NT; q++) en[q] = len12[L[q - 1].g][x[q] >> 8];
  m[0] = chain_next(S, g, en[0], x[0], i, CH_NONE);
  m[0] = 2 * (i < span ? m[0] : i);
#pragma unroll
  for (int q = 1; q < NT; q++) { m[q] = chain_next(S, L[q - 1].g, en[q], x[q], i, CH_NONE2); m[q] = 2 * (i < CH_WIN ? m[q] : i); }
  ch_st(A, 0, i, m[0]);
#pragma unroll
  for (int q = 1; q < NT; q++) ch_st(L[q - 1].t, 0, i, m[q]);
  __syncthreads();
  uint32_t hop = 0;
#pragma unroll
  for (int lv = 1; lv <= 4; lv++) {
    m[0] = ch_ld(A, lv - 1, m[0]);
#pragma unroll
    for (int q = 1; q < NT; q++) m[q] = ch_ld(L[q - 1].t, lv - 1, m[q]);
    ch_st(A, lv, i, m[0]);
#pragma unroll
    for (int q = 1; q < NT; q++) ch_st(L[q - 1].t, lv, i, m[q]);
    __syncthreads();
    if (lv == 1) hop = ch_ld(A, 1, 0);
    if (lv == 4) hop = ch_ld(A, 4, hop);
  }
  // The last round: A's next^32 (one hop is left for it), but the later tables' next^50 = next^2 . next^16 . next^32 outright: two more
  // gathers here (every position at once) instead of two more hops each behind the barrier (one after the other).
  m[0] = ch_ld(A, 4, m[0]);
#pragma unroll
  for (int q = 1; q < NT; q++) m[q] = ch_ld(L[q - 1].t, 4, m[q]);
  ch_st(A, 5, i, m[0]);
#pragma unroll
  for (int q = 1; q < NT; q++) m[q] = ch_ld(L[q - 1].t, 4, m[q]);
#pragma unroll
  for (int q = 1; q < NT; q++) m[q] = ch_ld(L[q - 1].t, 1, m[q]);
#pragma unroll
  for (int q = 1; q < NT; q++) ch_st(L[q - 1].t, 5, i, m[q]);
  __syncthreads();
  // Where the groups end.  A chain that has left its positions STAYS on the value it left with, and a value equal to the number of
  // positions may be such a stop in the middle of the group: only a value below it is the end of 50 codes for sure -- except on the
  // whole span, whose last position nothing but 50 codes of the longest length reach.  A group that starts outside its table's
  // positions is looked up at CH_NONE2, which maps to itself.
  e[0] = ch_ld(A, 5, hop) >> 1;
  e[1] = e[2] = e[3] = CH_NONE2;
  bool known = e[0] < span || (whole && e[0] == span);
  uint32_t at = e[0];                            // where the group in front ends, in bits of the step
#pragma unroll
  for (int q = 1; q < NT; q++) {
    const bool in = known && at >= L[q - 1].start && at - L[q - 1].start < CH_WIN;
    e[q] = ch_ld(L[q - 1].t, 5, 2 * (in ? at - L[q - 1].start : CH_NONE2)) >> 1;
    known = e[q] < CH_WIN;
    at = L[q - 1].start + e[q];
  }
}
// The same for group k alone on its whole span (two positions per thread)
__device__ __forceinline__ uint32_t chain_table_full(const DecShared& S, const uint8_t (*len12)[4096], const uint32_t* wbuf, uint16_t (*A)[CH_ARR], uint32_t i, uint32_t o0, int g, uint32_t span) {
  const uint32_t j = i + CH_T;
  const uint32_t x0 = chain_bits(wbuf, o0 + i), x1 = chain_bits(wbuf, o0 + j);
  uint32_t m0 = chain_next(S, g, len12[g][x0 >> 8], x0, i, CH_NONE), m1 = chain_next(S, g, len12[g][x1 >> 8], x1, j, CH_NONE);
  m0 = 2 * (i < span ? m0 : i); m1 = 2 * (j < span ? m1 : j);
  ch_st(A, 0, i, m0); ch_st(A, 0, j, m1);
  __syncthreads();
  uint32_t hop = 0;
#pragma unroll
  for (int lv = 1; lv <= 5; lv++) {
    m0 = ch_ld(A, lv - 1, m0); m1 = ch_ld(A, lv - 1, m1);
    ch_st(A, lv, i, m0); ch_st(A, lv, j, m1);
    __syncthreads();
    if (lv == 1) hop = ch_ld(A, 1, 0);
    if (lv == 4) hop = ch_ld(A, 4, hop);
  }
  return hop;
}

// One workgroup per row: the symbols in front of the end-of-block symbol, 4096 per tile, front to back.
//   RUNA (0) / RUNB (1) are the bijective base-2 digits of a zero-rank run (:1621-1638): digit d adds (sym + 1) << d bytes.  The
//   reference keeps the digit weight in an int32 that it shifts left: the 32nd digit of a run adds (sym + 1) * -2^31, leaves the
//   weight 0, and with it the run is forgotten (the flush at :1643 tests the weight); a 33rd digit starts a fresh run.  So the
//   digit of a run symbol is its position in the run mod 32, and a symbol with digit 31 takes back what the 31 in front of it added.
//   rank symbols (>= 2) emit one byte each and leave as op (rank - 1, output offset); the bytes must fit the block (:1647, :1663).
constexpr int SO_PT = 8;                       // symbols per thread (a tile is a dozen barriers whatever it holds: 0.58 / 0.47 / 0.87 ms per 100 MB with 4 / 8 / 16)
constexpr uint32_t SO_TILE = 1024 * SO_PT, SO_KG = SO_TILE / GROUP_SYMS + 2;      // a tile's symbols lie in SO_KG groups at most

// ---------------------------------------------------------------- 5. RLE1 expansion (dec_unrle1.hip)
// A block is expanded in tiles of UR_TILE bytes, one workgroup of 1024 threads each.  RleCarry: the state at a tile's start (start of
// the current stretch, its carried bit, output bytes so far), one per chain block and tile: written by phase B, read by phase C.
constexpr int UR_BPT = 16;                          // bytes per thread: the ten-step function scan over the 1024 threads is most of a tile, whatever the bytes per thread (4 bytes: 1.05 ms per 100 MB for the length pass)
constexpr uint32_t UR_TILE = 1024 * UR_BPT;
struct RleCarry { uint32_t cur_start, cur_c0, out_base, pad; };

// batch_dec.hip: the batch forms, launched on stream s (input k of the group: bytes [st[k], en[k]); per candidate: cend = the end
// of its input, cdsz = 100000 x that input's largest level; rlim: one word per row of the row batch)
void launch_magic_scan_batch(hipStream_t s, const uint8_t* d_in, const uint32_t* d_st, const uint32_t* d_en, uint32_t count, uint64_t bytes,
                             Cand* d_cand, uint32_t cap, uint32_t* d_count);
void launch_block_decode_batch(hipStream_t s, const uint8_t* d_in, const uint32_t* d_cend, const uint32_t* d_cdsz, uint32_t* d_rlim, const Cand* d_cand, uint32_t nc, uint32_t rows, uint32_t dsz,
                               RowTab* d_tabs, uint8_t* d_sel, uint32_t* d_gstart, uint8_t* d_l0, BlockOut* d_bo, uint32_t r0, uint32_t group_tiles,
                               uint16_t* d_syms, uint32_t sym_stride, uint32_t sym_groups, uint8_t* d_ops, uint32_t* d_opoff, uint32_t ops_stride, uint32_t* d_nops);

// dec_device.hip: the device-resident source (cjs_bzip2_decompress_device).  Input k = d_in[off[k] .. off[k+1]).
struct DevHdr { uint8_t h[4]; uint32_t level; };      // first 4 bytes (zeros past the end), largest member level found (multistream)
constexpr int EOS_REC = 12;                            // bytes kept per end-of-stream candidate, from byte (bit + 48) / 8 on
void launch_dev_headers(hipStream_t s, const uint8_t* d_in, const uint64_t* d_off, uint32_t count, bool multistream, uint64_t b0, uint64_t b1, DevHdr* d_hdr);
void launch_dev_eos_bytes(hipStream_t s, const uint8_t* d_in, const uint64_t* d_tab, uint32_t n, uint8_t* d_out);
// a batch group's upload: piece i = len bytes of d_in from src to dst + dst (4-byte aligned), zeros up to the next whole word
struct GatherPiece { uint64_t src; uint32_t dst, len; };
constexpr size_t GATHER_PIECE = 65536;                 // bytes per piece of an input (a multiple of 4)
void launch_dev_gather(hipStream_t s, const uint8_t* d_in, const GatherPiece* d_pc, uint32_t npieces, uint8_t* dst);

}  // namespace cjs
