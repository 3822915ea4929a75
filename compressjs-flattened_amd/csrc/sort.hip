// sort.hip -- the lines of a text in device memory ordered by content (cjs_text_sort[_device]): a string sort in
// rounds of 7 bytes over line records; only line numbers, counts and the text asked for leave the GPU.  The rule is sort_plan.h
// (no HIP).
//   sl_count    per 4 KiB tile of the text: its newlines                                  (sl_scan: their exclusive prefix sums)
//   sl_starts   per newline: the start of the line behind it, at the newline's rank + 1; a line's length is start[i + 1] - 1 -
//               start[i] (a tail without a newline gets a virtual one: start[lines] = n + 1)
//   sl_words    per active line: its round word at depth d, kept a second time for the regroup, its dense index as the value
//   (radix_passes over the word, 64 bits; from round 1 on sl_gkeys and radix_passes over the group ordinal: stable by (group, word))
//   sl_heads    per dense slot: the sorted line to order[its slot] (the place step), the head flag from its dense neighbour's
//               (group, word), the done / active flag; per tile of SL_TILE the active lines and the active groups
//   sl_active   the active slots compacted in ascending order into the next round's dense arrays: slot, line, group ordinal
//   sl_hcount / sl_groups / sl_emit   after the last round: the runs of equal lines, and the first cap entries at scanned ranks
//   sl_lsum / sl_offs / sl_gather     the text: the 64-bit exclusive scan of len + 1 over the emitted lines, then a workgroup per
//               4 KiB of OUTPUT that finds each byte's line in LDS, so one long line and many empty ones cost the same
// No atomics: every rank comes from a scan.  The host waits once per round for one scalar, the lines still active.
#include "cjs_internal.h"
#include "host.h"
#include "prims.hpp"
#include "dec_engine.h"      // on_device
#include "range_engine.h"    // drained
#include "sort.h"

using namespace cjs;

namespace cjs {

// the newlines among the 16 bytes at shifted offset q0 of the aligned base A0, of which [lo, hi) are the text's: bit i = byte q0 + i
__device__ __forceinline__ uint32_t sl_chunk_newlines(const uint8_t* __restrict__ A0, uint64_t q0, uint64_t lo, uint64_t hi) {
  uint32_t m = 0;
  if (q0 >= lo && q0 + 16 <= hi) {
    const uint4 v = *reinterpret_cast<const uint4*>(A0 + q0);
    const uint32_t x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 16; i++) m |= (((x[i >> 2] >> (8 * (i & 3))) & 0xFFu) == 0x0Au ? 1u : 0u) << i;
  } else {
    for (int i = 0; i < 16; i++) { const uint64_t q = q0 + i; if (q >= lo && q < hi && A0[q] == 0x0A) m |= 1u << i; }
  }
  return m;
}

__global__ __launch_bounds__(256) void sl_count(const uint8_t* __restrict__ A0, uint64_t lo, uint64_t hi, uint64_t* __restrict__ tc) {
  __shared__ uint32_t sm[4];
  const uint64_t q0 = (uint64_t)blockIdx.x * SL_TEXT_TILE + threadIdx.x * 16;
  const uint32_t c = q0 < hi ? __popc(sl_chunk_newlines(A0, q0, lo, hi)) : 0;
  const uint32_t t = block_sum<256, uint32_t>(c, sm);
  if (threadIdx.x == 0) tc[blockIdx.x] = t;
}

// One workgroup: cnt[0 .. nt) and, if given, aux[0 .. nt) -> their exclusive prefix sums, the totals to scal[s_cnt] / scal[s_aux];
// cnt[nt] / aux[nt] get the totals too.  last: the text's last byte; scal[SL_TAIL] = it is no newline (nullptr: left alone).
__global__ __launch_bounds__(256) void sl_scan(uint64_t* __restrict__ cnt, uint64_t* __restrict__ aux, uint64_t nt, uint64_t* __restrict__ scal, int s_cnt, int s_aux,
                                               const uint8_t* __restrict__ last) {
  __shared__ uint64_t sm[4];
  uint64_t run = 0, arun = 0;
  for (uint64_t b = 0; b < nt; b += 256) {
    const uint64_t i = b + threadIdx.x, c = i < nt ? cnt[i] : 0, a = aux && i < nt ? aux[i] : 0;
    uint64_t tot, atot;
    const uint64_t ex = block_excl_sum<256, uint64_t>(c, sm, tot), ax = block_excl_sum<256, uint64_t>(a, sm, atot);
    if (i < nt) { cnt[i] = run + ex; if (aux) aux[i] = arun + ax; }
    run += tot; arun += atot;
  }
  if (threadIdx.x == 0) {
    cnt[nt] = run; scal[s_cnt] = run;
    if (aux) { aux[nt] = arun; scal[s_aux] = arun; }
    if (last) scal[SL_TAIL] = *last != 0x0A;
  }
}

// start[rank + 1] of every newline; start[0] = 0 and, with a tail, start[lines] = n + 1 (lines = newlines + tail)
__global__ __launch_bounds__(256) void sl_starts(const uint8_t* __restrict__ A0, uint64_t lo, uint64_t hi, const uint64_t* __restrict__ tc, uint64_t lines, uint32_t tail,
                                                 uint32_t* __restrict__ start) {
  __shared__ uint32_t sm[4];
  const uint64_t q0 = (uint64_t)blockIdx.x * SL_TEXT_TILE + threadIdx.x * 16;
  uint32_t m = q0 < hi ? sl_chunk_newlines(A0, q0, lo, hi) : 0, tot;
  uint64_t r = tc[blockIdx.x] + block_excl_sum<256, uint32_t>(__popc(m), sm, tot);
  for (; m; m &= m - 1, r++) {
    const uint64_t p = q0 + (__ffs(m) - 1) - lo;      // the newline's offset in the text
    if (r + 1 <= lines) start[r + 1] = (uint32_t)(p + 1);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) { start[0] = 0; if (tail) start[lines] = (uint32_t)(hi - lo + 1); }
}

// The round word (sl_word of sort_plan.h) of the line at text[s .. s + len) at depth d.  Reads no byte outside [text, text + n):
// two aligned 8-byte loads where both lie inside, byte loads of the line's own bytes near the two ends of the text.
__device__ __forceinline__ uint64_t sl_word_at(const uint8_t* __restrict__ text, uint64_t n, uint32_t s, uint32_t len, uint64_t d) {
  if (d >= len) return 0;
  const uint64_t left = len - d;
  const uint32_t k = left < 7 ? (uint32_t)left : 7u;
  const uint8_t* A = text + s + d;
  const uintptr_t a = (uintptr_t)A, base = a & ~(uintptr_t)7;
  uint64_t v = 0;
  if (base >= (uintptr_t)text && base + 16 <= (uintptr_t)text + n) {
    const uint64_t l = *reinterpret_cast<const uint64_t*>(base), h = *reinterpret_cast<const uint64_t*>(base + 8);
    const uint32_t sh = (uint32_t)(a & 7) * 8;
    v = sh ? (l >> sh) | (h << (64 - sh)) : l;
  } else {
    for (uint32_t i = 0; i < k; i++) v |= (uint64_t)A[i] << (8 * i);
  }
  const uint64_t be = (__builtin_bswap64(v) >> 8) & (~0ull << (8 * (7 - k)));      // bytes 0 .. 6 big-endian, those past k cleared
  return be << 8 | k;
}

// aline == nullptr (round 0): dense index j is line j
__global__ __launch_bounds__(256) void sl_words(const uint8_t* __restrict__ text, uint64_t n, const uint32_t* __restrict__ start, const uint32_t* __restrict__ aline,
                                                uint32_t na, uint64_t d, uint64_t* __restrict__ key, uint64_t* __restrict__ wsave, uint32_t* __restrict__ val) {
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= na) return;
  const uint32_t line = aline ? aline[j] : (uint32_t)j, s = start[line], len = start[line + 1] - 1 - s;
  const uint64_t w = sl_word_at(text, n, s, len, d);
  key[j] = w; wsave[j] = w; val[j] = (uint32_t)j;
}

// the second sort's key of a word-sorted slot: the group ordinal of the line that stands there
__global__ __launch_bounds__(256) void sl_gkeys(const uint32_t* __restrict__ agrp, const uint32_t* __restrict__ val, uint32_t na, uint32_t* __restrict__ gk) {
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (j < na) gk[j] = agrp[val[j]];
}

// this thread's flag of round r of its tile -> the number of set flags of the tile in front of it (rounds in slot order)
__device__ __forceinline__ uint32_t sl_rank(uint32_t f, uint32_t& run, uint32_t* sm) {
  uint32_t tot;
  const uint32_t ex = block_excl_sum<256, uint32_t>(f, sm, tot);
  const uint32_t r = run + ex;
  run += tot;
  return r;
}

// Dense slot jj of the sorted active set: its line goes to order[its slot]; it heads a group iff its (group, word) differs from
// its dense neighbour's; its group is active iff it has a second member and the word has not ended.  aslot / aline / agrp ==
// nullptr (round 0): the identity, the identity, one group.
__global__ __launch_bounds__(256) void sl_heads(const uint32_t* __restrict__ val, const uint64_t* __restrict__ wsave, const uint32_t* __restrict__ aslot,
                                                const uint32_t* __restrict__ aline, const uint32_t* __restrict__ agrp, uint32_t na, uint32_t* __restrict__ order,
                                                uint8_t* __restrict__ head, uint8_t* __restrict__ aflag, uint64_t* __restrict__ nact, uint64_t* __restrict__ ngrp) {
  __shared__ uint32_t sm[4];
  const uint64_t base = (uint64_t)blockIdx.x * SL_TILE;
  uint32_t act = 0, grp = 0;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const uint64_t jj = base + (uint64_t)r * 256 + threadIdx.x;
    if (jj >= na) continue;
    const uint32_t j = val[jj], g = agrp ? agrp[jj] : 0;
    const uint64_t w = wsave[j];
    const bool h = jj == 0 || (agrp && agrp[jj - 1] != g) || wsave[val[jj - 1]] != w;
    const bool hn = jj + 1 >= na || (agrp && agrp[jj + 1] != g) || wsave[val[jj + 1]] != w;
    const bool a = (w & 0xFF) == 7 && !(h && hn);
    const uint32_t slot = aslot ? aslot[jj] : (uint32_t)jj;
    order[slot] = aline ? aline[j] : j;
    head[slot] = h;
    aflag[jj] = (uint8_t)(h | (a ? 2 : 0));
    act += a; grp += a && h;
  }
  const uint32_t ta = block_sum<256, uint32_t>(act, sm), tg = block_sum<256, uint32_t>(grp, sm);
  if (threadIdx.x == 0) { nact[blockIdx.x] = ta; ngrp[blockIdx.x] = tg; }
}

// nact / ngrp scanned: the next round's dense arrays (an active group's first member is a head, so its ordinal counts itself)
__global__ __launch_bounds__(256) void sl_active(const uint8_t* __restrict__ aflag, const uint32_t* __restrict__ val, const uint32_t* __restrict__ aslot,
                                                 const uint32_t* __restrict__ aline, uint32_t na, const uint64_t* __restrict__ nact, const uint64_t* __restrict__ ngrp,
                                                 uint32_t* __restrict__ nslot, uint32_t* __restrict__ nline, uint32_t* __restrict__ ngroup) {
  __shared__ uint32_t sm[4];
  const uint64_t base = (uint64_t)blockIdx.x * SL_TILE;
  const uint64_t a0 = nact[blockIdx.x], g0 = ngrp[blockIdx.x];
  uint32_t run = 0, grun = 0;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const uint64_t jj = base + (uint64_t)r * 256 + threadIdx.x;
    const uint32_t f = jj < na ? aflag[jj] : 0, a = f >> 1, ah = a & f;
    const uint32_t rk = sl_rank(a, run, sm), gr = sl_rank(ah, grun, sm);
    if (!a) continue;
    const uint64_t at = a0 + rk;                  // (at < the active lines <= na)
    const uint32_t j = val[jj];
    nslot[at] = aslot ? aslot[jj] : (uint32_t)jj;
    nline[at] = aline ? aline[j] : j;
    ngroup[at] = (uint32_t)(g0 + gr + ah - 1);    // the heads at or in front of it, less one
  }
}

// per tile of slots: the heads, and the bytes of their lines with a newline each
__global__ __launch_bounds__(256) void sl_hcount(const uint8_t* __restrict__ head, const uint32_t* __restrict__ order, const uint32_t* __restrict__ start, uint32_t L,
                                                 uint64_t* __restrict__ nhead, uint64_t* __restrict__ nbytes) {
  __shared__ uint64_t sm[4];
  const uint64_t base = (uint64_t)blockIdx.x * SL_TILE;
  uint64_t heads = 0, bytes = 0;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const uint64_t i = base + (uint64_t)r * 256 + threadIdx.x;
    if (i >= L || !head[i]) continue;
    const uint32_t line = order[i];
    heads++; bytes += start[line + 1] - start[line];
  }
  const uint64_t h = block_sum<256, uint64_t>(heads, sm), b = block_sum<256, uint64_t>(bytes, sm);
  if (threadIdx.x == 0) { nhead[blockIdx.x] = h; nbytes[blockIdx.x] = b; }
}

__global__ __launch_bounds__(256) void sl_groups(const uint8_t* __restrict__ head, uint32_t L, const uint64_t* __restrict__ nhead, uint32_t* __restrict__ gpos) {
  __shared__ uint32_t sm[4];
  const uint64_t base = (uint64_t)blockIdx.x * SL_TILE;
  const uint64_t g0 = nhead[blockIdx.x];
  uint32_t run = 0;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const uint64_t i = base + (uint64_t)r * 256 + threadIdx.x;
    const uint32_t f = i < L && head[i];
    const uint32_t rk = sl_rank(f, run, sm);
    if (f) gpos[g0 + rk] = (uint32_t)i;      // (g0 + rk < the heads <= L)
  }
}

// Slot i of group g = [gs, ge): without UNIQUE it is entry i, or under REVERSE entry (L - ge) + (i - gs); with UNIQUE the head is
// entry g, or under REVERSE nd - 1 - g.  Entries below m are written: the line number, the count, the line for the gather.
__global__ __launch_bounds__(256) void sl_emit(const uint8_t* __restrict__ head, const uint32_t* __restrict__ order, const uint32_t* __restrict__ gpos, uint32_t L,
                                               uint64_t nd, const uint64_t* __restrict__ nhead, uint32_t flags, uint64_t base_line, uint64_t m,
                                               uint64_t* __restrict__ lines_out, uint64_t* __restrict__ counts_out, uint32_t* __restrict__ eline) {
  __shared__ uint32_t sm[4];
  const uint64_t base = (uint64_t)blockIdx.x * SL_TILE;
  const uint64_t g0 = nhead[blockIdx.x];
  uint32_t run = 0;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const uint64_t i = base + (uint64_t)r * 256 + threadIdx.x;
    const uint32_t f = i < L && head[i];
    const uint32_t rk = sl_rank(f, run, sm);
    if (i >= L) continue;
    const uint64_t g = g0 + rk + f - 1;          // (slot 0 is a head: g >= 0)
    if (g >= nd) continue;
    const uint64_t gs = gpos[g], ge = g + 1 < nd ? gpos[g + 1] : L;
    uint64_t pos, cnt = 1;
    if (flags & CJS_SORT_UNIQUE) {
      if (!f) continue;
      pos = flags & CJS_SORT_REVERSE ? nd - 1 - g : g; cnt = ge - gs;
    } else pos = flags & CJS_SORT_REVERSE ? (L - ge) + (i - gs) : i;
    if (pos >= m) continue;
    const uint32_t line = order[i];
    lines_out[pos] = base_line + line;
    if (counts_out) counts_out[pos] = cnt;
    eline[pos] = line;
  }
}

// per tile of emitted lines: their bytes with a newline each
__global__ __launch_bounds__(256) void sl_lsum(const uint32_t* __restrict__ eline, const uint32_t* __restrict__ start, uint64_t m, uint64_t* __restrict__ tsum) {
  __shared__ uint64_t sm[4];
  const uint64_t base = (uint64_t)blockIdx.x * SL_TILE;
  uint64_t bytes = 0;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const uint64_t i = base + (uint64_t)r * 256 + threadIdx.x;
    if (i < m) { const uint32_t line = eline[i]; bytes += start[line + 1] - start[line]; }
  }
  const uint64_t b = block_sum<256, uint64_t>(bytes, sm);
  if (threadIdx.x == 0) tsum[blockIdx.x] = b;
}
// ... and every emitted line's offset in the text; off[m] = the total
__global__ __launch_bounds__(256) void sl_offs(const uint32_t* __restrict__ eline, const uint32_t* __restrict__ start, uint64_t m, const uint64_t* __restrict__ tsum,
                                               uint64_t* __restrict__ off) {
  __shared__ uint64_t sm[4];
  const uint64_t base = (uint64_t)blockIdx.x * SL_TILE;
  uint64_t run = tsum[blockIdx.x];
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const uint64_t i = base + (uint64_t)r * 256 + threadIdx.x;
    uint64_t b = 0, tot;
    if (i < m) { const uint32_t line = eline[i]; b = start[line + 1] - start[line]; }
    const uint64_t ex = block_excl_sum<256, uint64_t>(b, sm, tot);
    if (i < m) { off[i] = run + ex; if (i + 1 == m) off[m] = run + ex + b; }
    run += tot;
  }
}

// the largest k in [0, m) with off[k] <= x (off[0] = 0 <= x)
__device__ __forceinline__ uint64_t sl_line_of(const uint64_t* __restrict__ off, uint64_t m, uint64_t x) {
  uint64_t lo = 0, hi = m;      // off[lo] <= x < off[hi]
  while (hi - lo > 1) { const uint64_t mid = lo + (hi - lo) / 2; if (off[mid] <= x) lo = mid; else hi = mid; }
  return lo;
}

// A workgroup per SL_OUT_TILE bytes of the output.  The lines that reach into the tile (at most SL_OUT_TILE: a line has a byte at
// least, its newline) stand in LDS with their offset in the tile and their start in the text; thread t writes bytes t, t + 256,
// ... of the tile (coalesced), finding each byte's line by a binary search in LDS.  Reads stay inside the lines, writes inside
// [out, out + total).
__global__ __launch_bounds__(256) void sl_gather(const uint8_t* __restrict__ text, const uint32_t* __restrict__ start, const uint32_t* __restrict__ eline,
                                                 const uint64_t* __restrict__ off, uint64_t m, uint64_t total, uint8_t* __restrict__ out) {
  __shared__ uint32_t s_rel[SL_OUT_TILE];      // the line's first byte, relative to the tile (entry 0: unused, see s_first)
  __shared__ uint32_t s_src[SL_OUT_TILE];
  __shared__ uint64_t s_k[2];
  const uint64_t B = (uint64_t)blockIdx.x * SL_OUT_TILE, E = B + SL_OUT_TILE < total ? B + SL_OUT_TILE : total;
  if (threadIdx.x == 0) s_k[0] = sl_line_of(off, m, B);
  if (threadIdx.x == 64) s_k[1] = sl_line_of(off, m, E - 1);
  __syncthreads();
  const uint64_t k0 = s_k[0], k1 = s_k[1];
  const uint32_t cnt = (uint32_t)(k1 - k0 + 1);
  const uint64_t first = off[k0], end = off[k1 + 1];
  for (uint32_t i = threadIdx.x; i < cnt; i += 256) {
    s_rel[i] = i ? (uint32_t)(off[k0 + i] - B) : 0u;
    s_src[i] = start[eline[k0 + i]];
  }
  __syncthreads();
  for (uint64_t b = B + threadIdx.x; b < E; b += 256) {
    const uint32_t rel = (uint32_t)(b - B);
    uint32_t lo = 0, hi = cnt;      // line lo starts at or in front of b, line hi behind it
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (s_rel[mid] <= rel) lo = mid; else hi = mid; }
    const uint64_t in_line = lo ? rel - s_rel[lo] : b - first;
    const uint64_t next = lo + 1 < cnt ? B + s_rel[lo + 1] : end;
    out[b] = b + 1 == next ? (uint8_t)0x0A : text[(uint64_t)s_src[lo] + in_line];
  }
}

int sort_count(hipStream_t s, SortCount& c, const uint8_t* d_text, size_t n, uint64_t* lines, SortStats& st) {
  const uint64_t a = (uintptr_t)d_text & 15u;
  const uint8_t* A0 = d_text - a;
  const unsigned nt = (unsigned)((a + n + SL_TEXT_TILE - 1) / SL_TEXT_TILE);
  uint64_t scal[2] = {0, 0};
  hipLaunchKernelGGL(sl_count, dim3(nt), dim3(256), 0, s, A0, a, a + (uint64_t)n, c.tc);
  hipLaunchKernelGGL(sl_scan, dim3(1), dim3(256), 0, s, c.tc, (uint64_t*)nullptr, (uint64_t)nt, c.scal, (int)SL_NL, (int)SL_SPARE, d_text + (n - 1));
  int rc = hipGetLastError() != hipSuccess || hipMemcpyAsync(scal, c.scal, 16, hipMemcpyDeviceToHost, s) != hipSuccess ? CJS_E_HIP : 0;
  if ((rc = drained(s, rc))) return rc;
  st.d2h += 16;
  if (scal[SL_NL] > n || scal[SL_TAIL] > 1) return CJS_E_HIP;      // (what sizes the launches behind it is checked, not trusted)
  *lines = scal[SL_NL] + scal[SL_TAIL];
  return 0;
}

int sort_run(hipStream_t s, SortWork& w, const SortCount& c, const SortCall& q, uint64_t lines, uint64_t* text_n, cjs_bz_sort_info* info, SortStats& st) {
  if (!lines || lines > w.lines || lines > SL_MAX_LINES) return drained(s, CJS_E_INVALID_ARG);
  const uint32_t L = (uint32_t)lines;
  const uint8_t* d_text = q.d_text;
  const uint64_t n = q.n, a = (uintptr_t)d_text & 15u;
  const unsigned tt = (unsigned)((a + n + SL_TEXT_TILE - 1) / SL_TEXT_TILE);
  uint64_t scal[SL_SCALARS] = {0};
  if (hipMemcpyAsync(scal, c.scal, 16, hipMemcpyDeviceToHost, s) != hipSuccess) return drained(s, CJS_E_HIP);      // (the tail flag again: the caller's copy is gone)
  CJS_TRY(drained(s, 0));
  st.d2h += 16;
  const uint32_t tail = (uint32_t)scal[SL_TAIL];
  if (scal[SL_NL] + tail != lines) return CJS_E_HIP;
  hipLaunchKernelGGL(sl_starts, dim3(tt), dim3(256), 0, s, d_text - a, a, a + n, (const uint64_t*)c.tc, lines, tail, w.start);
  info->n_lines = lines;
  // ---- the rounds
  uint32_t na = L;
  const uint32_t *aslot = nullptr, *aline = nullptr, *agrp = nullptr;
  int nxt = 0;
  uint64_t rounds = 0;
  for (;; rounds++) {
    const unsigned per = (unsigned)(((uint64_t)na + 255) / 256), nt = (unsigned)sl_tiles(na);
    int cur = 0;
    hipLaunchKernelGGL(sl_words, dim3(per), dim3(256), 0, s, d_text, n, (const uint32_t*)w.start, aline, na, 7 * rounds, w.key[0], w.wsave, w.val[0]);
    int rc = radix_passes<uint64_t>(s, w.rs, w.key[0], w.val[0], w.key[1], w.val[1], cur, na, 0, 64);
    const uint32_t* perm = w.val[cur];
    if (!rc && agrp) {
      // the groups' ordinals are below na / 2 + 1 (an active group has two members at least); whole digits, as the passes sort them
      const int bits = (bits_for(na / 2) + 7) & ~7;
      int c2 = 0;
      hipLaunchKernelGGL(sl_gkeys, dim3(per), dim3(256), 0, s, agrp, perm, na, w.gk[0]);
      rc = radix_passes<uint32_t>(s, w.rs, w.gk[0], w.val[cur], w.gk[1], w.val[1 - cur], c2, na, 0, bits ? bits : 8);
      perm = c2 ? w.val[1 - cur] : w.val[cur];
    }
    if (rc) return drained(s, rc);
    hipLaunchKernelGGL(sl_heads, dim3(nt), dim3(256), 0, s, perm, (const uint64_t*)w.wsave, aslot, aline, agrp, na, w.order, w.head, w.aflag, w.tcnt, w.taux);
    hipLaunchKernelGGL(sl_scan, dim3(1), dim3(256), 0, s, w.tcnt, w.taux, (uint64_t)nt, w.scal, (int)SL_NACT, (int)SL_NGRP, (const uint8_t*)nullptr);
    hipLaunchKernelGGL(sl_active, dim3(nt), dim3(256), 0, s, (const uint8_t*)w.aflag, perm, aslot, aline, na, (const uint64_t*)w.tcnt, (const uint64_t*)w.taux,
                       w.dense[nxt][0], w.dense[nxt][1], w.dense[nxt][2]);
    rc = hipGetLastError() != hipSuccess || hipMemcpyAsync(scal + SL_NACT, w.scal + SL_NACT, 8, hipMemcpyDeviceToHost, s) != hipSuccess ? CJS_E_HIP : 0;
    if ((rc = drained(s, rc))) return rc;
    st.d2h += 8;
    const uint64_t act = scal[SL_NACT];
    if (act > na || act == 1) return CJS_E_HIP;
    if (!act) { rounds++; break; }
    na = (uint32_t)act;
    aslot = w.dense[nxt][0]; aline = w.dense[nxt][1]; agrp = w.dense[nxt][2];
    nxt = 1 - nxt;
  }
  info->rounds = rounds;
  // ---- the runs of equal lines
  const unsigned lt = (unsigned)sl_tiles(L);
  hipLaunchKernelGGL(sl_hcount, dim3(lt), dim3(256), 0, s, (const uint8_t*)w.head, (const uint32_t*)w.order, (const uint32_t*)w.start, L, w.tcnt, w.taux);
  hipLaunchKernelGGL(sl_scan, dim3(1), dim3(256), 0, s, w.tcnt, w.taux, (uint64_t)lt, w.scal, (int)SL_ND, (int)SL_UBYTES, (const uint8_t*)nullptr);
  hipLaunchKernelGGL(sl_groups, dim3(lt), dim3(256), 0, s, (const uint8_t*)w.head, L, (const uint64_t*)w.tcnt, w.gpos);
  int rc = hipGetLastError() != hipSuccess || hipMemcpyAsync(scal + SL_ND, w.scal + SL_ND, 16, hipMemcpyDeviceToHost, s) != hipSuccess ? CJS_E_HIP : 0;
  if ((rc = drained(s, rc))) return rc;
  st.d2h += 16;
  const uint64_t nd = scal[SL_ND];
  if (!nd || nd > L) return CJS_E_HIP;
  const bool uniq = q.flags & CJS_SORT_UNIQUE;
  info->n_distinct = nd;
  info->n_out = uniq ? nd : L;
  info->text_bytes = uniq ? scal[SL_UBYTES] : n + tail;
  const uint64_t m = std::min<uint64_t>(q.cap, info->n_out);
  if (text_n) *text_n = 0;
  if (!m) return 0;
  hipLaunchKernelGGL(sl_emit, dim3(lt), dim3(256), 0, s, (const uint8_t*)w.head, (const uint32_t*)w.order, (const uint32_t*)w.gpos, L, nd, (const uint64_t*)w.tcnt,
                     q.flags, q.base, m, q.d_lines, q.d_counts, w.eline);
  if (!q.text) return drained(s, hipGetLastError() != hipSuccess ? (int)CJS_E_HIP : 0);
  // ---- the text of the emitted lines
  const unsigned mt = (unsigned)sl_tiles(m);
  hipLaunchKernelGGL(sl_lsum, dim3(mt), dim3(256), 0, s, (const uint32_t*)w.eline, (const uint32_t*)w.start, m, w.taux);
  hipLaunchKernelGGL(sl_scan, dim3(1), dim3(256), 0, s, w.taux, (uint64_t*)nullptr, (uint64_t)mt, w.scal, (int)SL_TEXT, (int)SL_SPARE, (const uint8_t*)nullptr);
  hipLaunchKernelGGL(sl_offs, dim3(mt), dim3(256), 0, s, (const uint32_t*)w.eline, (const uint32_t*)w.start, m, (const uint64_t*)w.taux, w.off);
  rc = hipGetLastError() != hipSuccess || hipMemcpyAsync(scal + SL_TEXT, w.scal + SL_TEXT, 8, hipMemcpyDeviceToHost, s) != hipSuccess ? CJS_E_HIP : 0;
  if ((rc = drained(s, rc))) return rc;
  st.d2h += 8;
  const uint64_t total = scal[SL_TEXT];
  if (total < m || total > n + 1) return CJS_E_HIP;
  *text_n = (size_t)total;
  uint8_t* d_out = nullptr;
  CJS_TRY(q.text(total, &d_out));
  hipLaunchKernelGGL(sl_gather, dim3((unsigned)((total + SL_OUT_TILE - 1) / SL_OUT_TILE)), dim3(256), 0, s, d_text, (const uint32_t*)w.start, (const uint32_t*)w.eline,
                     (const uint64_t*)w.off, m, total, d_out);
  return drained(s, hipGetLastError() != hipSuccess ? (int)CJS_E_HIP : 0);
}

}  // namespace cjs

namespace {

int sort_checks(const void* text, size_t n, uint32_t flags, const void* lines_out, size_t cap, bool text_ptr, bool text_n_ptr, cjs_bz_sort_info* info) {
  clear_detail();
  CJS_TRY(sl_args(text, n, flags, lines_out, cap, text_ptr, text_n_ptr, info));
  sl_info_clear(info);
  return (uint64_t)n > SL_MAX_BYTES ? CJS_E_UNSUPPORTED : 0;
}

void sort_debug(const char* form, size_t n, const cjs_bz_sort_info* info, const SortStats& st) {
  if (!env_debug()) return;
  fprintf(stderr, "[cjs sort] %s text: %zu bytes, %llu lines, %llu distinct, %llu out, %llu rounds, H2D %llu D2H %llu\n", form, n, (unsigned long long)info->n_lines,
          (unsigned long long)info->n_distinct, (unsigned long long)info->n_out, (unsigned long long)info->rounds, (unsigned long long)st.h2d,
          (unsigned long long)st.d2h);
}

}  // namespace

extern "C" int cjs_text_sort(const uint8_t* text, size_t n, uint32_t flags, uint64_t* lines_out, uint64_t* counts_out, size_t cap, uint8_t** text_out, size_t* text_n,
                             cjs_bz_sort_info* info, const cjs_opts* opts) {
  CJS_GUARD_BEGIN
  CJS_TRY(sort_checks(text, n, flags, lines_out, cap, text_out != nullptr, text_n != nullptr, info));
  if (text_out) { *text_out = nullptr; *text_n = 0; }
  HostBuf host;
  if (!n) {
    if (text_out && !(*text_out = HostBuf(1).release())) return CJS_E_OUT_OF_MEMORY;
    return 0;
  }
  CallDevice cd;
  CJS_TRY(cd.select(opts));
  DevBuf d_text(n);
  Arena ca;
  SortCount c;
  if (!d_text.p) return CJS_E_OUT_OF_MEMORY;
  CJS_TRY(ca.init_pooled(SortCount::bytes_needed(n)));
  CJS_TRY(c.carve(ca, n));
  Stream s;
  CJS_HIP_TRY(hipStreamCreate(s.put()));
  SortStats st;
  if (hipMemcpyAsync(d_text.p, text, n, hipMemcpyHostToDevice, s) != hipSuccess) return drained(s, CJS_E_HIP);
  st.h2d += n;
  uint64_t L = 0;
  CJS_TRY(sort_count(s, c, (const uint8_t*)d_text.p, n, &L, st));
  int rc = 0;
  size_t tn = 0;
  if (L) {
    const size_t room = (size_t)std::min<uint64_t>(cap, L);
    Arena wa;
    SortWork w;
    DevBuf d_lines(8 * std::max<size_t>(room, 1)), d_counts(counts_out ? 8 * std::max<size_t>(room, 1) : 8), d_out(text_out ? n + 1 : 1);
    if (!d_lines.p || !d_counts.p || !d_out.p) return CJS_E_OUT_OF_MEMORY;
    CJS_TRY(wa.init_pooled(SortWork::bytes_needed((size_t)L)));
    CJS_TRY(w.carve(wa, (size_t)L));
    SortCall q;
    q.d_text = (const uint8_t*)d_text.p; q.n = n; q.flags = flags; q.d_lines = (uint64_t*)d_lines.p; q.d_counts = counts_out ? (uint64_t*)d_counts.p : nullptr; q.cap = cap;
    if (text_out) q.text = [&](uint64_t, uint8_t** p) { *p = (uint8_t*)d_out.p; return 0; };      // (the text is n + 1 bytes at most)
    rc = sort_run(s, w, c, q, L, &tn, info, st);
    const size_t m = (size_t)std::min<uint64_t>(cap, info->n_out);
    if (!rc && text_out && !(host = HostBuf(std::max<size_t>(tn, 1)))) rc = CJS_E_OUT_OF_MEMORY;
    if (!rc && m && (hipMemcpyAsync(lines_out, d_lines.p, 8 * m, hipMemcpyDeviceToHost, s) != hipSuccess ||
                     (counts_out && hipMemcpyAsync(counts_out, d_counts.p, 8 * m, hipMemcpyDeviceToHost, s) != hipSuccess))) rc = CJS_E_HIP;
    if (!rc && text_out && tn && hipMemcpyAsync(host.p, d_out.p, tn, hipMemcpyDeviceToHost, s) != hipSuccess) rc = CJS_E_HIP;
    rc = drained(s, rc);
    st.d2h += 8 * m * (counts_out ? 2 : 1) + (text_out ? tn : 0);
  } else if (text_out && !(host = HostBuf(1))) rc = CJS_E_OUT_OF_MEMORY;
  if (rc) return rc;
  if (text_out) { *text_out = host.release(); *text_n = tn; }
  sort_debug("host", n, info, st);
  return 0;
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

extern "C" int cjs_text_sort_device(const uint8_t* d_text, size_t n, uint32_t flags, uint64_t* d_lines_out, uint64_t* d_counts_out, size_t cap, uint8_t* d_text_out,
                                    size_t text_cap, size_t* text_n, cjs_bz_sort_info* info, const cjs_opts* opts) {
  CJS_GUARD_BEGIN
  CJS_TRY(sort_checks(d_text, n, flags, d_lines_out, cap, text_n != nullptr, text_n != nullptr, info));
  if ((!d_text_out && text_cap) || (!text_n && d_text_out)) return CJS_E_INVALID_ARG;
  if (((uintptr_t)d_lines_out & 7u) || ((uintptr_t)d_counts_out & 7u)) return CJS_E_INVALID_ARG;
  if (text_n) *text_n = 0;
  if (!n) return 0;
  CallDevice cd;
  CJS_TRY(cd.select(opts));
  if (!on_device(d_text, cd.dev) || (cap && !on_device(d_lines_out, cd.dev)) || (cap && d_counts_out && !on_device(d_counts_out, cd.dev)) ||
      (d_text_out && !on_device(d_text_out, cd.dev))) return CJS_E_INVALID_ARG;      // (no host pointer reaches a kernel)
  Arena ca;
  SortCount c;
  CJS_TRY(ca.init_pooled(SortCount::bytes_needed(n)));
  CJS_TRY(c.carve(ca, n));
  Stream s;
  CJS_HIP_TRY(hipStreamCreate(s.put()));
  SortStats st;
  uint64_t L = 0;
  CJS_TRY(sort_count(s, c, d_text, n, &L, st));
  if (!L) { sort_debug("device", n, info, st); return 0; }
  Arena wa;
  SortWork w;
  CJS_TRY(wa.init_pooled(SortWork::bytes_needed((size_t)L)));
  CJS_TRY(w.carve(wa, (size_t)L));
  SortCall q;
  q.d_text = d_text; q.n = n; q.flags = flags; q.d_lines = d_lines_out; q.d_counts = d_counts_out; q.cap = cap;
  if (text_n) q.text = [&](uint64_t need, uint8_t** p) { *p = d_text_out; return need > text_cap ? (int)CJS_E_OUTPUT_TOO_SMALL : 0; };
  size_t tn = 0;
  const int rc = sort_run(s, w, c, q, L, &tn, info, st);
  if (text_n) *text_n = tn;
  if (!rc) sort_debug("device", n, info, st);
  return rc;
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

extern "C" int cjs_stage_text_sort(const uint8_t* text, size_t n, uint32_t flags, uint64_t* lines_out, uint64_t* counts_out, size_t cap, cjs_bz_sort_info* info) {
  CJS_GUARD_BEGIN
  return sl_sort_host(text, n, flags, lines_out, counts_out, cap, info);
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_INVALID_ARG)
}
