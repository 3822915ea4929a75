// bz_stage2.h -- the per-candidate kernels of block decode (bz_chain, bz_group_syms, bz_sym_ops; decode.hip stage 2b).
// decode.hip includes this file twice:
//   BZ_BATCH 0  cjs_bzip2_decompress: one stream; every read and the end-bit clamp stop at its end n.
//   BZ_BATCH 1  cjs_bzip2_decompress_batch: the kernels get the suffix _batch, and every read and the end-bit clamp stop at the end
//               of the candidate's OWN input (cend[c], bytes from the group's start): past it they read the zero bits the
//               reference's reader yields behind a lone file.  bz_chain leaves that end in RowTab::pad for the stages behind it.
//               The block-size limits are the input's own as well (cdsz[c] = 100000 x the largest level of the candidate's
//               input, what its single call would use, not the group's): the header's origPointer test, the symbol cap
//               (rlim[row] + 4096, left by bz_chain for bz_group_syms) and the rank-op and byte limits of bz_sym_ops.
// (One text for both forms, and the first one exactly the single-stream kernels: an inlined template body was not
// instruction-identical to them.)
#if BZ_BATCH
#define BZ_NAME(x) x##_batch
#define BZ_CEND , const uint32_t* __restrict__ cend, const uint32_t* __restrict__ cdsz, uint32_t* __restrict__ rlim
#define BZ_GS_EXTRA , const uint32_t* __restrict__ rlim
#define BZ_SO_EXTRA , const uint32_t* __restrict__ cdsz
#else
#define BZ_NAME(x) x
#define BZ_CEND
#define BZ_GS_EXTRA
#define BZ_SO_EXTRA
#endif

__device__ int BZ_NAME(dec_prologue)(DecShared& S, BitReader& r, uint32_t dbuf_size, uint32_t& crc, uint32_t& orig, uint32_t& sym_total,
                            uint32_t& group_count, uint32_t& n_sel, uint8_t* __restrict__ selectors /* global, room for 32768 */, uint32_t* __restrict__ selp) {
  int err = 0;
  sym_total = 0; group_count = 0; n_sel = 0; orig = 0;
  const int lane = lane_id();
  if (lane == 0) {                                           // header (:1440-1493)
    crc = r.get(16) << 16; crc |= r.get(16);
    if (r.get(1)) err = CJS_E_OBSOLETE_INPUT;
    orig = r.get(24);
    if (!err && orig > dbuf_size) err = CJS_E_DATA_ERROR;
    const uint32_t t = r.get(16);
    for (int i = 0; i < 256; i++) S.sym_to_byte[i] = 0;
    for (int i = 0; i < 16; i++) if (t & (1u << (15 - i))) {
      const uint32_t k = r.get(16);
      for (int j = 0; j < 16; j++) if (k & (1u << (15 - j))) S.sym_to_byte[sym_total++] = (uint8_t)(i * 16 + j);
    }
    group_count = r.get(3);
    if (!err && (group_count < 2 || group_count > 6)) err = CJS_E_DATA_ERROR;
    n_sel = r.get(15);
    if (!err && n_sel == 0) err = CJS_E_DATA_ERROR;
  }
  err = __builtin_amdgcn_readfirstlane(err);
  group_count = __builtin_amdgcn_readfirstlane(group_count); n_sel = __builtin_amdgcn_readfirstlane(n_sel); sym_total = __builtin_amdgcn_readfirstlane(sym_total);
  uint64_t pos = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)r.pos) | ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(r.pos >> 32)) << 32);
  if (!err) {
    // Selector list (:1487-1493): n_sel unary numbers (ones closed by a zero).  Every lane takes 32 bits of a 2048-bit stretch:
    // its zeros are selector ends, the ones in front of a zero (back to the previous zero, which may sit in the lane before) the
    // value.  A value may equal group_count (the reference tests the count BEFORE it reads on: j ones pass for j <= group_count,
    // and its list holds zeros behind the groups); one more is an error.
    for (uint32_t i = lane; i < (n_sel + 7) / 8; i += 64) selp[i] = 0;
    __builtin_amdgcn_wave_barrier();
    const uint64_t nbytes = (r.nbits + 7) >> 3;
    uint32_t done = 0, carry = 0; int bad = 0; uint64_t endpos = pos;
    while (done < n_sel) {
      const uint64_t bp = pos + 32u * (uint32_t)lane;
      const uint32_t w0 = load_be32(r.p, nbytes, bp >> 5), w1 = load_be32(r.p, nbytes, (bp >> 5) + 1);
      const uint32_t v = (uint32_t)(((((uint64_t)w0 << 32) | w1) << (bp & 31)) >> 32);
      const uint32_t nz = (uint32_t)__builtin_popcount(~v);
      const uint32_t incl = wave_incl_sum(nz), excl = incl - nz;
      const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
      const uint32_t t1 = v == 0xFFFFFFFFu ? 32u : (uint32_t)__builtin_ctz(~v);      // ones at the end of my word (32: all of it -- more than any value)
      uint32_t pend = (uint32_t)__shfl_up((int)t1, 1, 64);
      if (lane == 0) pend = carry;
      uint32_t z = ~v, k = done + excl; int prevb = -1 - (int)pend;
      while (z && k < n_sel) {
        const int bidx = __builtin_clz(z);
        const uint32_t j = (uint32_t)(bidx - prevb - 1);
        if (j > group_count) bad = 1;
        else atomicOr(&selp[k >> 3], j << (4u * (k & 7u)));
        if (k + 1 == n_sel) endpos = bp + (uint32_t)bidx + 1u;
        z &= ~(0x80000000u >> bidx); prevb = bidx; k++;
      }
      if (done + total >= n_sel) {                                       // the lane that holds the last selector knows where the list ends
        const uint64_t m = __ballot(done + incl >= n_sel);
        const int l = (int)__builtin_ctzll(m);
        endpos = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)endpos, l) | ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(endpos >> 32), l) << 32);
        done = n_sel;
      } else { done += total; carry = (uint32_t)__builtin_amdgcn_readlane((int)t1, 63); pos += 2048; }
    }
    if (__ballot(bad != 0)) err = CJS_E_DATA_ERROR;
    __builtin_amdgcn_wave_barrier();
    if (!err) {
      // Move-to-front over the values, the list as nibbles of one register.  A stretch of the list acts on the positions as a
      // permutation whatever they hold: every lane composes its stretch's (from the identity), a scan composes those in front of each
      // lane, and a second walk from the list the lane really starts with writes the selectors.  (Position group_count holds the
      // zero of the reference's zero-initialised list: a value equal to the count reads it, and moves it.)
      const uint32_t cs = (((n_sel + 63u) >> 6) + 7u) & ~7u;             // values per lane: whole words of selp
      const uint32_t c0 = min((uint32_t)lane * cs, n_sel), c1 = min(c0 + cs, n_sel);
      uint32_t R = 0x76543210u, wv = 0;
      for (uint32_t i = c0; i < c1; i++) {
        if ((i & 7u) == 0) wv = selp[i >> 3];
        R = nib_to_front(R, wv & 15u); wv >>= 4;
      }
      uint32_t I = R;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)I, d, 64);
        if (lane >= d) I = nib_compose(up, I);
      }
      uint32_t E = (uint32_t)__shfl_up((int)I, 1, 64);
      if (lane == 0) E = 0x76543210u;
      uint32_t st = 0;
      for (uint32_t i = 0; i < group_count; i++) st |= i << (4u * i);
      st = nib_compose(st, E);
      for (uint32_t i = c0; i < c1; i++) {
        if ((i & 7u) == 0) wv = selp[i >> 3];
        const uint32_t j = wv & 15u; wv >>= 4;
        selectors[i] = (uint8_t)((st >> (4u * j)) & 15u);
        st = nib_to_front(st, j);
      }
    }
    pos = endpos > r.nbits ? r.nbits : endpos;
  }
  if (!err) {
    // Code lengths (:1500-1520): per table 5 bits, then per symbol a run of (1, direction) pairs closed by a 0.  Behind a 0 and behind
    // a direction bit stands a control bit, so in a run of ones the bits alternate control / direction from the run's first (a control
    // bit): what a lane's first bit is follows from the parity of the ones in front of it.  Every lane walks 32 bits of a 2048-bit
    // stretch twice: once for its count of symbol ends and its sum of steps, and -- with the sums of the lanes in front -- once more
    // to write the lengths.  The reference tests the running length wherever it has changed (and where a table starts): 1 .. 20.
    const uint64_t nbytes = (r.nbits + 7) >> 3;
    const uint32_t sym_count0 = sym_total + 2;
    int bad = 0;
    for (uint32_t g = 0; g < group_count && !__ballot(bad != 0); g++) {
      int cur0;
      { const uint32_t w0 = load_be32(r.p, nbytes, pos >> 5), w1 = load_be32(r.p, nbytes, (pos >> 5) + 1);
        cur0 = (int)((((((uint64_t)w0 << 32) | w1) << (pos & 31)) >> 59)); pos += 5; }
      if (cur0 < 1 || cur0 > 20) bad = 1;
      uint32_t done = 0, par_in = 0;
      for (;;) {
        const uint64_t bp = pos + 32u * (uint32_t)lane;
        const uint32_t w0 = load_be32(r.p, nbytes, bp >> 5), w1 = load_be32(r.p, nbytes, (bp >> 5) + 1);
        const uint32_t v = (uint32_t)(((((uint64_t)w0 << 32) | w1) << (bp & 31)) >> 32);
        const uint32_t t1 = v == 0xFFFFFFFFu ? 32u : (uint32_t)__builtin_ctz(~v);
        const uint64_t m_ao = __ballot(v == 0xFFFFFFFFu), m_par = __ballot((t1 & 1u) != 0);
        const uint64_t below = ~m_ao & ((1ull << lane) - 1ull);
        const uint32_t par = below ? (uint32_t)((m_par >> (63 - __builtin_clzll(below))) & 1ull) : par_in;      // 1: my first bit is a direction bit
        uint32_t state = par, ne = 0; int nd = 0;
        for (int b = 31; b >= 0; b--) {
          const uint32_t bit = (v >> b) & 1u;
          if (state) { nd += bit ? -1 : 1; state = 0; }
          else if (bit) state = 1;
          else ne++;
        }
        const uint32_t ie = wave_incl_sum(ne); const int id = wave_incl_sum(nd);
        const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)ie, 63);
        uint32_t idx = done + ie - ne; int cur = cur0 + id - nd; uint64_t endpos = 0;
        state = par;
        for (int b = 31; b >= 0 && idx < sym_count0; b--) {
          const uint32_t bit = (v >> b) & 1u;
          if (state) { cur += bit ? -1 : 1; if (cur < 1 || cur > 20) bad = 1; state = 0; }
          else if (bit) state = 1;
          else { S.length[g][idx] = (uint8_t)cur; if (++idx == sym_count0) endpos = bp + (uint32_t)(32 - b); }
        }
        if (__ballot(bad != 0)) break;                                   // (the reference stops at the first length out of range; so must a stretch of ones)
        if (done + total >= sym_count0) {                                // the lane that wrote the last length knows where the table ends
          const int l = (int)__builtin_ctzll(__ballot(done + ie >= sym_count0));
          pos = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)endpos, l) | ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(endpos >> 32), l) << 32);
          break;
        }
        done += total; cur0 += __builtin_amdgcn_readlane(id, 63);
        if (~m_ao) par_in = (uint32_t)((m_par >> (63 - __builtin_clzll(~m_ao))) & 1ull);
        pos += 2048;
      }
    }
    if (__ballot(bad != 0)) err = CJS_E_DATA_ERROR;
  }
  if (lane == 0) r.pos = pos > r.nbits ? r.nbits : pos;
  // lane 0's results become wave-uniform scalars (readfirstlane, not a shuffle: the compiler must KNOW they are uniform,
  // or the whole symbol loop is compiled as divergent code under exec masks)
  err = __builtin_amdgcn_readfirstlane(err);
  sym_total = __builtin_amdgcn_readfirstlane(sym_total); group_count = __builtin_amdgcn_readfirstlane(group_count);
  n_sel = __builtin_amdgcn_readfirstlane(n_sel);
  const uint32_t sym_count = sym_total + 2;
  __builtin_amdgcn_wave_barrier();
  if (!err) {
    // canonical tables: lane g builds table g -- a counting sort of the symbols by length, then the first codes
    if ((uint32_t)lane < group_count) {
      const int g = lane;
      for (int i = 0; i < 22; i++) { S.cnt[g][i] = 0; S.first[g][i] = 0; S.start[g][i] = 0; }
      int mn = 20, mx = 1;
      for (uint32_t i = 0; i < sym_count; i++) { const int l = S.length[g][i]; S.cnt[g][l]++; mn = l < mn ? l : mn; mx = l > mx ? l : mx; }
      S.minlen[g] = (uint8_t)mn; S.maxlen[g] = (uint8_t)mx;
      uint32_t code = 0, at = 0; uint16_t fillp[22];
      for (int l = mn; l <= mx; l++) {
        S.first[g][l] = code; S.start[g][l] = (uint16_t)at; fillp[l] = (uint16_t)at;
        at += S.cnt[g][l];
        code = (code + S.cnt[g][l]) << 1;
      }
      for (uint32_t i = 0; i < sym_count; i++) S.bysym[g][fillp[S.length[g][i]]++] = (uint16_t)i;
      for (int l = 1; l <= 20; l++) {
        const uint32_t lj = l < mn ? 0u : l <= mx ? (S.first[g][l] + S.cnt[g][l]) << (20 - l) : (1u << 20);
        S.limp[g][l] = l == 20 ? (mx == 20 ? lj : (S.first[g][mx] + S.cnt[g][mx]) << (20 - mx)) : (l < mx ? lj : (l >= mn ? (1u << 20) : 0u));
      }
      S.limp[g][0] = 0;
    }
  }
  __builtin_amdgcn_wave_barrier();
  crc = __builtin_amdgcn_readfirstlane(crc);
  orig = __builtin_amdgcn_readfirstlane(orig);
  r.pos = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)r.pos) | ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(r.pos >> 32)) << 32);   // (the builtin returns int: no sign extension of a low half >= 2^31)
  return err;
}

__global__ __launch_bounds__(CH_T) void BZ_NAME(bz_chain)(const uint8_t* __restrict__ in, uint64_t n, const Cand* __restrict__ cands, uint32_t ncand, uint32_t dbuf_size,
                                                 RowTab* __restrict__ tabs, uint8_t* __restrict__ sel_all, uint32_t* __restrict__ gstart_all,
                                                 uint8_t* __restrict__ l0_all, BlockOut* __restrict__ outs, uint32_t row0 BZ_CEND) {
  __shared__ DecShared S;
  __shared__ uint32_t scratch[4 * CH_ARR / 2 + 12 * CH_ARR2 / 2 + CH_WORDS + 2];         // the prologue's selector values (4096 words), then the chain's arrays
  uint16_t (*A)[CH_ARR] = reinterpret_cast<uint16_t (*)[CH_ARR]>(scratch);                     // group k: next^(2^lv), lv = 0 .. 5, in four arrays (ch_slot)
  uint16_t (*B)[CH_ARR2] = reinterpret_cast<uint16_t (*)[CH_ARR2]>(scratch + 4 * CH_ARR / 2);                    // groups k + 1, k + 2, k + 3: four arrays each
  uint32_t* wbuf = scratch + 4 * CH_ARR / 2 + 12 * CH_ARR2 / 2;
  __shared__ uint8_t len12[6][4096];            // code length by the next 12 bits (chain_next)
  __shared__ uint64_t s_pos;
  __shared__ uint32_t s_hdr[8];
  const uint32_t c = blockIdx.x;
  if (c >= ncand) return;
  const int tid = threadIdx.x, lane = tid & 63;
  if (cands[c].kind != 0) {                     // end-of-stream candidate: nothing to decode
    if (tid == 0) { BlockOut bo; bo.end_bit = cands[c].bit + 48; bo.count = 0; bo.orig = 0; bo.crc = 0; bo.err = 0; outs[c] = bo; }
    return;
  }
  const uint32_t row = cands[c].pad - row0;     // row of this batch's scratch
#if BZ_BATCH
  n = cend[c];                                  // (bytes from the group's start)
  dbuf_size = cdsz[c];
  if (tid == 0) rlim[row] = dbuf_size;
#endif
  RowTab& T = tabs[row];
  uint8_t* sel = sel_all + (size_t)row * MAX_SELECTORS;
  uint32_t* gstart = gstart_all + (size_t)row * (MAX_SELECTORS + 1);
  const uint64_t t_k0 = wall_clock64();
  if (tid < 64) {                               // wave 0: header, selectors, code lengths, tables
    BitReader r{in, n * 8, cands[c].bit + 48, 0, ~0ull >> 4};
    uint32_t sym_total = 0, group_count = 0, n_sel = 0, orig = 0, crc = 0;
    const int err = BZ_NAME(dec_prologue)(S, r, dbuf_size, crc, orig, sym_total, group_count, n_sel, sel, scratch);
    if (lane == 0) {
      s_hdr[0] = (uint32_t)err; s_hdr[1] = sym_total; s_hdr[2] = group_count; s_hdr[3] = n_sel; s_hdr[4] = crc; s_hdr[5] = orig;
      s_pos = r.pos;
    }
  }
  __threadfence_block();
  __syncthreads();
  const uint64_t t_hdr = wall_clock64();
#if BZ_BATCH
  (void)t_k0;                                   // (the phase clock is the single-stream form's)
#else
  if (tid == 0 && blockIdx.x == 0) g_dec_clk[5] = t_hdr - t_k0;
#endif
  const int herr = (int)s_hdr[0];
  const uint32_t group_count = s_hdr[2], n_sel = s_hdr[3];
  const uint64_t data_bit = s_pos;
  // the tables go to global memory for the symbol stage
  // ... with the 10-bit direct tables: entry x = the code that is a prefix of the 10 bits x, if it has one of <= 10 bits
  if (!herr) {
    for (uint32_t e = tid; e < group_count * 1024u; e += CH_T) {
      const uint32_t t = e >> 10, x = e & 1023u;
      const int mn = S.minlen[t], mx = S.maxlen[t];
      uint16_t v = 0;
      for (int l = mn; l <= 10 && l <= mx; l++) {
        const uint32_t k = (x >> (10 - l)) - S.first[t][l];              // (not below first: no shorter code matched)
        if (k < S.cnt[t][l]) { v = (uint16_t)((S.bysym[t][S.start[t][l] + k] << 5) | l); break; }
      }
      T.fast[t][x] = v;
    }
  }
  for (uint32_t i = tid; i < 6 * 22; i += CH_T) { (&T.first[0][0])[i] = (&S.first[0][0])[i]; (&T.cnt[0][0])[i] = (&S.cnt[0][0])[i]; (&T.start[0][0])[i] = (&S.start[0][0])[i]; }
  for (uint32_t i = tid; i < 6 * 260; i += CH_T) (&T.bysym[0][0])[i] = (&S.bysym[0][0])[i];
  if (tid < 8) { T.minlen[tid] = S.minlen[tid]; T.maxlen[tid] = S.maxlen[tid]; }
  for (int i = tid; i < 256; i += CH_T) l0_all[(size_t)row * 256 + i] = S.sym_to_byte[i];
  // 12-bit direct length tables.  The length rule is 1 + #{L in 1..19 : x20 >= limp[L]}, and a limit of a length <= 12 has its low 8
  // bits clear: the 12 bits x decide those; with all 12 below x the code is longer (or there is none) and the entry is 0.
  if (!herr) {
    for (uint32_t e = tid; e < group_count * 4096u; e += CH_T) {
      const uint32_t t = e >> 12, x = e & 4095u;
      uint32_t c = 0;
#pragma unroll
      for (int l = 1; l <= 12; l++) c += x >= (S.limp[t][l] >> 8) ? 1u : 0u;
      len12[t][x] = (uint8_t)(c == 12 ? 0u : (x << 8) < S.limp[t][20] ? c + 1 : CH_NOCODE);
    }
  }
  // (the positions behind the last a thread writes, once for every level)
  if (tid < 64) { for (int a = 0; a < 4; a++) A[a][CH_SPAN + tid] = (uint16_t)(2 * (CH_SPAN + tid)); for (int a = 0; a < 12; a++) B[a][CH_T + tid] = (uint16_t)(2 * (CH_T + tid)); }
  __syncthreads();
  uint32_t ok_groups = 0;
  if (!herr) {
    // Nothing the step's first instructions need comes from memory: the tables' shortest / longest lengths sit in registers (5 / 10 bits
    // each: the longest, and 50 x the shortest), and lane j of every wave holds the selectors kb + 8 j .. kb + 8 j + 7 as nibbles (15:
    // none) -- written by wave 0 above, visible after the barrier; 512 selectors per fill.
    uint32_t maxp = 0; uint64_t minp = 0;
    for (int t = 0; t < 6; t++) { minp |= (uint64_t)(GROUP_SYMS * ((uint32_t)S.minlen[t] & 31u)) << (10 * t); maxp |= ((uint32_t)S.maxlen[t] & 31u) << (5 * t); }
    maxp = (uint32_t)__builtin_amdgcn_readfirstlane((int)maxp);
    minp = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)minp) | ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(minp >> 32)) << 32);
    uint32_t kb = 0, sw = 0, lp = 0;
    uint32_t rel = 0, o0 = CH_WORDS * 32;          // bits from data_bit / from the window's first word to the step's first bit (o0 past the window: fill it)
    for (uint32_t k = 0; k < n_sel;) {
      if (k == 0 || k - kb >= 512 - 16) {          // (uniform) the next 512 selectors
        kb = k & ~7u;
        const uint32_t at = kb + 8u * (uint32_t)lane;
        uint64_t v = ~0ull;
        if (at < n_sel) v = *reinterpret_cast<const uint64_t*>(sel + at);                  // (the row is 8-byte aligned; bytes behind the list: masked)
        if (at + 8 > n_sel && at < n_sel) v |= ~0ull << (8u * (n_sel - at));
        v = (v | (v >> 4)) & 0x00FF00FF00FF00FFull; v = (v | (v >> 8)) & 0x0000FFFF0000FFFFull; v = v | (v >> 16);
        sw = (uint32_t)v;
      }
      const uint32_t kj = (uint32_t)__builtin_amdgcn_readfirstlane((int)(k - kb));
      const uint64_t sn = (((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)sw, (int)((kj >> 3) + 1)) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)sw, (int)(kj >> 3))) >> (4u * (kj & 7u));
      // Up to FOUR groups per step.  The tables next^1 .. next^32 of a group do not depend on where the group starts, only on its
      // code table and on the bit positions they cover.  So beside group k's tables from its known start (A) the same threads build
      // those of group k + 1 under ITS code table over CH_WIN positions from the earliest bit it can start at (50 x the shortest code
      // of group k's table), and of groups k + 2 and k + 3 likewise -- in the same rounds, behind the same barriers.  When the hops
      // on A have found where group k ends, the later tables are looked up there, one after the other.  The span that is safe for
      // any 50 codes (50 x the longest) is about five times what 50 codes of text take (~210 bits): the first attempt works on CH_WIN
      // positions; a group k that leaves them (or meets a position where no code starts) is worked out again, alone, on its whole
      // span; a later group that leaves its table's positions, or starts in front of them, simply is the first group of the next step.
      const int g = (int)(sn & 15u);
      const uint32_t n1 = (uint32_t)(sn >> 4) & 15u, n2 = (uint32_t)(sn >> 8) & 15u, n3 = (uint32_t)(sn >> 12) & 15u;
      const int g1 = n1 < 6 ? (int)n1 : -1, g2 = n2 < 6 ? (int)n2 : -1, g3 = n3 < 6 ? (int)n3 : -1;
      const uint32_t full_span = min(GROUP_SYMS * ((maxp >> (5 * g)) & 31u), CH_SPAN);
      const uint32_t base1 = (uint32_t)(minp >> (10 * g)) & 1023u;                          // group k + 1 starts at or behind this offset
      const uint32_t base2 = base1 + ((uint32_t)(minp >> (10 * min(n1, 5u))) & 1023u);       // ... group k + 2 at or behind this one
      const uint32_t base3 = base2 + ((uint32_t)(minp >> (10 * min(n2, 5u))) & 1023u);       // ... and group k + 3 here (no group: not used)
      if (o0 + 2 * CH_SPAN + 128 > CH_WORDS * 32) {                                         // (uniform) refill the bit window
        __syncthreads();
        const uint64_t pos = data_bit + rel, wbase = pos >> 5;
        for (uint32_t i = tid; i < CH_WORDS + 2; i += CH_T) wbuf[i] = load_be32(in, n, wbase + i);
        o0 = (uint32_t)(pos & 31u);
        __syncthreads();
      }
      const uint32_t i = (uint32_t)tid;
      // (where the later tables start: the earliest bit the group can start at, or -- lp = the bits of the last group -- half a group in
      // front of where groups of that length would put it, if that is more: its CH_WIN positions must hold the group's start AND end)
      const ChainLater L[3] = {{B, g1, min(base1, CH_SPAN)},
                               {B + 4, g2, min(max(base2, lp * 3 / 2), 2 * CH_SPAN - CH_T)},
                               {B + 8, g3, min(max(base3, lp * 5 / 2), 2 * CH_SPAN - CH_T)}};
      uint32_t span = min(full_span, CH_WIN), e[4];
      if (g3 >= 0) chain_tables<4>(S, len12, wbuf, A, L, i, o0, g, span, span == full_span, e);
      else if (g2 >= 0) chain_tables<3>(S, len12, wbuf, A, L, i, o0, g, span, span == full_span, e);
      else if (g1 >= 0) chain_tables<2>(S, len12, wbuf, A, L, i, o0, g, span, span == full_span, e);
      else chain_tables<1>(S, len12, wbuf, A, L, i, o0, g, span, span == full_span, e);
      uint32_t e0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)e[0]);
      const uint32_t e1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)e[1]), e2 = (uint32_t)__builtin_amdgcn_readfirstlane((int)e[2]), e3 = (uint32_t)__builtin_amdgcn_readfirstlane((int)e[3]);
      bool ok0 = e0 < span || (span == full_span && e0 == span);
      if (!ok0 && span < full_span) {              // (uniform) group k alone on its whole span
        span = full_span;
        e0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)ch_ld(A, 5, chain_table_full(S, len12, wbuf, A, i, o0, g, span))) >> 1;
        ok0 = e0 <= span;
      }
      if (tid == 0) gstart[k] = rel;
      ok_groups = k + 1;
      if (!ok0) break;                             // (uniform) a code of the group is undecodable: the symbol stage reports it -- or finds the end of the block in front of it
      // (a later group's end is known only if those in front of it are: chain_tables)
      uint32_t adv;
      if (e3 < CH_WIN) {                           // four groups
        if (tid == 0) { gstart[k + 1] = rel + e0; gstart[k + 2] = rel + L[0].start + e1; gstart[k + 3] = rel + L[1].start + e2; }
        ok_groups = k + 4;
        lp = L[2].start + e3 - (L[1].start + e2);
        adv = L[2].start + e3; k += 4;
      } else if (e2 < CH_WIN) {                    // three
        if (tid == 0) { gstart[k + 1] = rel + e0; gstart[k + 2] = rel + L[0].start + e1; }
        ok_groups = k + 3;
        lp = L[1].start + e2 - (L[0].start + e1);
        adv = L[1].start + e2; k += 3;
      } else if (e1 < CH_WIN) {                    // two
        if (tid == 0) gstart[k + 1] = rel + e0;
        ok_groups = k + 2;
        lp = L[0].start + e1 - e0;
        adv = L[0].start + e1; k += 2;
      } else { lp = e0; adv = e0; k += 1; }        // (the second group left its table's positions, met an undecodable position, or there was none: next step)
      rel += adv; o0 += adv;
    }
  }
#if BZ_BATCH
  (void)t_hdr;
#else
  if (tid == 0 && blockIdx.x == 0) { g_dec_clk[6] = wall_clock64() - t_hdr; g_dec_clk[7] = ok_groups; }
#endif
  if (tid == 0) {
    T.sym_total = s_hdr[1]; T.group_count = group_count; T.n_sel = n_sel; T.err = (uint32_t)herr; T.data_bit = data_bit; T.crc = s_hdr[4]; T.orig = s_hdr[5];
    T.ngroups_ok = ok_groups; T.pad = 0; T.eob_key = ~0ull; T.err_key = ~0ull;
#if BZ_BATCH
    T.pad = (uint32_t)n;                        // the input's end, for bz_group_syms and bz_sym_ops
#endif
  }
}

// one lane per group of 50 symbols; the block's tables in LDS
__global__ __launch_bounds__(256) void BZ_NAME(bz_group_syms)(const uint8_t* __restrict__ in, uint64_t n, RowTab* __restrict__ tabs, const uint8_t* __restrict__ sel_all,
                                                     const uint32_t* __restrict__ gstart_all, uint16_t* __restrict__ syms_all, uint32_t sym_stride, uint32_t sym_groups, uint32_t row0 BZ_GS_EXTRA) {
  __shared__ uint16_t fast[6][1024];
  __shared__ uint32_t first[6][22];
  __shared__ uint16_t cnt[6][22], start[6][22], bysym[6][260];
  __shared__ uint8_t maxlen[8];
  const uint32_t row = row0 + blockIdx.y;
  RowTab& T = tabs[row];
  const uint32_t ng = T.err ? 0u : T.ngroups_ok;
  if (blockIdx.x * 256u >= ng) return;
  const int tid = threadIdx.x;
  for (uint32_t i = tid; i < 6 * 1024; i += 256) (&fast[0][0])[i] = (&T.fast[0][0])[i];
  for (uint32_t i = tid; i < 6 * 22; i += 256) { (&first[0][0])[i] = (&T.first[0][0])[i]; (&cnt[0][0])[i] = (&T.cnt[0][0])[i]; (&start[0][0])[i] = (&T.start[0][0])[i]; }
  for (uint32_t i = tid; i < 6 * 260; i += 256) (&bysym[0][0])[i] = (&T.bysym[0][0])[i];
  if (tid < 8) maxlen[tid] = T.maxlen[tid];
  __syncthreads();
  const uint32_t k = blockIdx.x * 256u + tid;
  if (k >= ng) return;
#if BZ_BATCH
  n = T.pad;
  sym_stride = rlim[row] + 4096u;                // (the input's own symbol cap: dec_phase_a's sym_stride rule)
#endif
  const int g = sel_all[(size_t)row * MAX_SELECTORS + k];
  // (symbols 0 and 1 are RUNA and RUNB whatever the used map says: with no used byte there is NO end-of-block symbol, :1621 comes
  // before :1654, and the block is rejected when its selectors run out)
  const uint32_t last_rank = max(T.sym_total, 1u);
  const uint64_t data_bit = T.data_bit;
  uint64_t pos = data_bit + gstart_all[(size_t)row * (MAX_SELECTORS + 1) + k];
  // symbol j of group k is stored at [j][k]: the lanes of a wave (64 groups) write one line, not 64
  uint16_t* syms = syms_all + (size_t)row * sym_groups * GROUP_SYMS + k;
  const int mx = maxlen[g];
  // a 64-bit window on the stream: a code is at most 20 bits, so the cursor crosses at most one word per symbol (one load every
  // four or five symbols of text instead of two per symbol)
  uint64_t wdw = pos >> 5;
  uint32_t w0 = load_be32(in, n, wdw), w1 = load_be32(in, n, wdw + 1);
  for (uint32_t j = 0; j < GROUP_SYMS; j++) {
    const uint64_t idx = (uint64_t)k * GROUP_SYMS + j;
    if ((pos >> 5) != wdw) { wdw++; w0 = w1; w1 = load_be32(in, n, wdw + 1); }
    const uint32_t x20 = (uint32_t)(((((uint64_t)w0 << 32) | w1) << (pos & 31)) >> 44);
    uint32_t e = fast[g][x20 >> 10], sym = 0, len = 0;
    if (e) { sym = e >> 5; len = e & 31u; }
    else {
      for (int i = 11; i <= mx; i++) {
        const uint32_t q = (x20 >> (20 - i)) - first[g][i];
        if (q < cnt[g][i]) { len = (uint32_t)i; sym = bysym[g][start[g][i] + q]; break; }
      }
    }
    if (!len || idx >= sym_stride) { atomicMin(&T.err_key, (unsigned long long)idx << 32); break; }      // no code starts here (or more symbols than any block has room for)
    pos += len;
    if (sym > last_rank) { atomicMin(&T.eob_key, ((unsigned long long)idx << 32) | (unsigned long long)(uint32_t)(pos - data_bit)); break; }      // end of block (:1640)
    syms[(size_t)j * sym_groups] = (uint16_t)sym;
  }
}

__global__ __launch_bounds__(1024) void BZ_NAME(bz_sym_ops)(RowTab* __restrict__ tabs, const Cand* __restrict__ cands, uint32_t ncand, const uint16_t* __restrict__ syms_all,
                                                   uint32_t sym_groups, uint32_t dbuf_size, uint8_t* __restrict__ ops_all, uint32_t* __restrict__ opoff_all,
                                                   uint32_t ops_stride, uint32_t* __restrict__ nops_all, BlockOut* __restrict__ outs, uint32_t row0, uint64_t nbits BZ_SO_EXTRA) {
  __shared__ uint16_t st[SO_TILE + 32];          // the tile's symbols behind the last 32 of the tile in front
  __shared__ unsigned long long sm64[16];
  __shared__ uint32_t sm[16];
  __shared__ uint32_t mx[1024];
  const uint32_t c = blockIdx.x;
  if (c >= ncand || cands[c].kind != 0) return;
  const uint32_t row = cands[c].pad - row0;
  const RowTab& T = tabs[row];
  const int tid = threadIdx.x;
#if BZ_BATCH
  dbuf_size = cdsz[c];
  const uint32_t ops_cap = ((dbuf_size + 256u + 255u) & ~255u) - 1u;      // (the input's own ops_stride rule, <= the rows' stride)
#define BZ_OPS_CAP ops_cap
#else
#define BZ_OPS_CAP (ops_stride - 1u)
#endif
  int err = (int)T.err;
  const unsigned long long ek = T.eob_key, xk = T.err_key;
  if (!err && (ek == ~0ull || xk < ek)) err = CJS_E_DATA_ERROR;      // no end of block in the selectors' reach, or an undecodable code in front of it
  const uint32_t nsym = err ? 0u : (uint32_t)(ek >> 32);
  const uint16_t* syms = syms_all + (size_t)row * sym_groups * GROUP_SYMS;      // [symbol of the group][group] (bz_group_syms)
  uint8_t* ops = ops_all + (size_t)row * ops_stride;
  uint32_t* opoff = opoff_all + (size_t)row * ops_stride;
  unsigned long long off = 0;                    // bytes so far
  uint32_t j0 = 0, last_nonrun = 0;              // ops so far; (index of the last rank symbol so far) + 1
  if (tid < 32) st[tid] = 2;                     // in front of the first symbol: not a run
  for (uint32_t base = 0; base < nsym && !err; base += SO_TILE) {
    __syncthreads();
    {                                             // along the groups, symbol by symbol of the group
      const uint32_t k0 = base / GROUP_SYMS;
      constexpr int LR = (GROUP_SYMS * SO_KG + 1023) / 1024;
      uint32_t at[LR]; uint16_t v[LR];            // (all of a thread's loads on their way before the first is stored; fetching the tile
                                                  // behind during this one's work as well: 0.44 -> 0.70 ms)
#pragma unroll
      for (int q = 0; q < LR; q++) {
        const uint32_t u = (uint32_t)tid + 1024u * (uint32_t)q, j = u / SO_KG, k = k0 + (u - SO_KG * j), i = k * GROUP_SYMS + j;
        const bool in = u < GROUP_SYMS * SO_KG && i >= base && i < base + SO_TILE;
        at[q] = in ? 32u + i - base : ~0u;
        v[q] = in && i < nsym ? syms[(size_t)j * sym_groups + k] : (uint16_t)2;
      }
#pragma unroll
      for (int q = 0; q < LR; q++) if (at[q] != ~0u) st[at[q]] = v[q];
    }
    __syncthreads();
    // position in the run: i - (index of the last rank symbol in front of i) - 1, by a max scan of (index + 1) of the rank symbols
    uint32_t lastb = 0;
#pragma unroll
    for (int q = 0; q < SO_PT; q++) { const uint32_t i = base + (uint32_t)tid * (uint32_t)SO_PT + q; if (i < nsym && st[32 + tid * SO_PT + q] >= 2) lastb = i + 1; }
    const uint32_t incl = block_incl_max<1024>(lastb, sm);
    mx[tid] = incl;
    __syncthreads();
    uint32_t prevnr = tid ? mx[tid - 1] : 0u;
    const uint32_t tile_last = mx[1023];
    __syncthreads();
    if (prevnr < last_nonrun) prevnr = last_nonrun;
    long long cb[SO_PT]; unsigned long long mine = 0; uint32_t nops = 0;
#pragma unroll
    for (int q = 0; q < SO_PT; q++) {
      const uint32_t i = base + (uint32_t)tid * (uint32_t)SO_PT + q, sy = st[32 + tid * SO_PT + q];
      cb[q] = 0;
      if (i < nsym) {
        if (sy >= 2) { cb[q] = 1; nops++; prevnr = i + 1; }
        else {
          const uint32_t d = (i - prevnr) & 31u;
          if (d < 31) cb[q] = (long long)(sy + 1u) << d;
          else { long long t = 0; for (uint32_t b = 1; b <= 31; b++) t += (long long)((uint32_t)st[32 + tid * SO_PT + q - b] + 1u) << (31u - b); cb[q] = -t; }
        }
      }
      mine += (unsigned long long)cb[q];
    }
    unsigned long long tot;
    unsigned long long ex = off + block_excl_sum<1024>(mine, sm64, tot);
    uint32_t ntot;
    uint32_t jx = j0 + block_excl_sum<1024>(nops, sm, ntot);
#pragma unroll
    for (int q = 0; q < SO_PT; q++) {
      const uint32_t i = base + (uint32_t)tid * (uint32_t)SO_PT + q, sy = st[32 + tid * SO_PT + q];
      if (i < nsym && sy >= 2) {
        if (jx < BZ_OPS_CAP && ex < 0xFFFFFFFFull) { ops[jx] = (uint8_t)(sy - 1u); opoff[jx] = (uint32_t)ex; }      // rank symbol s reads list slot s - 1 (:1664)
        jx++;
      }
      ex += (unsigned long long)cb[q];
    }
    off += tot; j0 += ntot;                       // (off may hold digits of a run that is still open: the byte limit is tested at the end)
    if (tile_last > last_nonrun) last_nonrun = tile_last;
    if (j0 >= BZ_OPS_CAP) err = CJS_E_DATA_ERROR;                           // (uniform) more rank symbols than the block has bytes
    __syncthreads();
    if (tid < 32) st[tid] = st[SO_TILE + tid];   // the last 32 symbols stay in front of the next tile
  }
  // Offsets at rank symbols never decrease, so every "fits the block" test of the reference (:1647 before a flush, :1663 before
  // a literal) passes iff the final byte count does
  if (!err && off > dbuf_size) err = CJS_E_DATA_ERROR;
  if (!err && T.orig >= off) err = CJS_E_DATA_ERROR;                            // :1677
  if (tid == 0) {
    if (err) { j0 = 0; off = 0; }
    opoff[j0] = (uint32_t)off;                   // the end-of-block pseudo op: where the output ends
    nops_all[row] = j0;
    BlockOut bo;
    const uint64_t endb = T.data_bit + (uint32_t)ek;
#if BZ_BATCH
    nbits = (uint64_t)T.pad * 8;
#endif
    bo.end_bit = err ? 0 : (endb > nbits ? nbits : endb);
    bo.count = err ? 0u : (uint32_t)off; bo.orig = T.orig; bo.crc = T.crc; bo.err = err;
    outs[c] = bo;
  }
}

#undef BZ_NAME
#undef BZ_CEND
#undef BZ_GS_EXTRA
#undef BZ_SO_EXTRA
#undef BZ_OPS_CAP
