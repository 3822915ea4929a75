// lines.hip -- the line table of an indexed .bz2 stream (cjs_bzip2_lines_*): the third consumer of the pass engine of
// the indexed entry points (range_engine.h).  Every decoded inverse-BWT batch is looked at where it stands expanded in device
// scratch; four bytes per block (the build) or eight per question leave the GPU.
//   ln_count    per 16 KiB tile of a block: the number of newlines in it
//   ln_scan     per block: the exclusive scan of its tile counts, the block's total
//   ln_select   per locate question (block, r): the decoded offset behind the r-th newline of the block
//   ln_rank     per number question (block, p): the newlines among the first p bytes of the block
// A tile is 16 KiB of one block, counted from the block's first byte (wherever that stands in the scratch): it never spans two.
#include "range_engine.h"
#include "bz_lines.h"
#include <algorithm>
#include <stdlib.h>
#include <string.h>

using namespace cjs;

namespace cjs {

constexpr uint32_t LN_TILE = 16384;                        // bytes of a tile (a multiple of a row)
constexpr uint32_t LN_ROW = 1024;                          // a row = the 64 x 16 bytes a wave looks at at once
static_assert(LN_ROW == 64 * 16 && LN_TILE % LN_ROW == 0, "a tile is whole rows of one 16-byte vector per lane");

struct LnBlk { uint64_t src, off; uint32_t len, tile0; };      // len bytes at device address src, decoded offset off; its first tile
struct LnAsk { uint32_t blk, arg; };                       // blk: which LnBlk; arg: r (1-based) of a locate, p of a number question

__host__ __device__ __forceinline__ uint32_t ln_tiles(uint32_t len) { return (len + LN_TILE - 1) / LN_TILE; }

// a tile's bytes as bounded aligned vectors (nothing outside the tile, so nothing outside the block, is read)
using LnSpan = RgSpan;

__global__ __launch_bounds__(256) void ln_count(const LnBlk* __restrict__ blks, uint32_t nblk, uint32_t* __restrict__ cnt) {
  __shared__ uint32_t sm[4];
  const uint32_t t = blockIdx.x;
  const LnBlk g = rg_seg_of(blks, nblk, t);
  const uint32_t p0 = (t - g.tile0) * LN_TILE;
  const LnSpan S = rg_span(g.src + p0, min(LN_TILE, g.len - p0));
  uint32_t c = 0;
  for (uint32_t v = threadIdx.x; v < S.nvec; v += 256) c += ln_count16(rg_vec(S, v));
  const uint32_t total = block_sum<256, uint32_t>(c, sm);
  if (threadIdx.x == 0) cnt[t] = total;
}

// block blockIdx.x: the counts of its tiles -> their exclusive prefix sums, tot = their sum
__global__ __launch_bounds__(256) void ln_scan(const LnBlk* __restrict__ blks, uint32_t* __restrict__ cnt, uint32_t* __restrict__ tot) {
  __shared__ uint32_t sm[4];
  const LnBlk g = blks[blockIdx.x];
  const uint32_t nt = ln_tiles(g.len);
  uint32_t* c = cnt + g.tile0;
  uint32_t run = 0;
  for (uint32_t b = 0; b < nt; b += 256) {
    const uint32_t i = b + threadIdx.x, v = i < nt ? c[i] : 0;
    uint32_t sum;
    const uint32_t ex = block_excl_sum<256, uint32_t>(v, sm, sum);
    if (i < nt) c[i] = run + ex;
    run += sum;
  }
  if (threadIdx.x == 0) tot[blockIdx.x] = run;
}

// One wave per question: the tile with ex < r <= ex + cnt by bisection of the block's scanned counts, then that tile row by row:
// the lanes' counts, their inclusive sums, the first lane that reaches what is left of r, the j-th newline of its 16 bytes.
// ans = the decoded offset of that newline + 1; ~0 for an r the block does not have (the host sees that from tot as well).
__global__ __launch_bounds__(256) void ln_select(const LnBlk* __restrict__ blks, const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ tot,
                                                 const LnAsk* __restrict__ asks, uint32_t nask, uint64_t* __restrict__ ans) {
  const uint32_t q = blockIdx.x * 4 + wave_id();
  if (q >= nask) return;
  const LnAsk A = asks[q];
  const LnBlk g = blks[A.blk];
  const uint32_t r = A.arg;
  if (r == 0 || r > tot[A.blk]) { if (lane_id() == 0) ans[q] = ~0ull; return; }
  const uint32_t* ex = cnt + g.tile0;
  uint32_t lo = 0, hi = ln_tiles(g.len);                                    // the last tile with ex < r
  while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (ex[mid] < r) lo = mid; else hi = mid; }
  uint32_t rem = r - ex[lo];
  const uint32_t p0 = lo * LN_TILE;
  const LnSpan S = rg_span(g.src + p0, min(LN_TILE, g.len - p0));
  for (uint32_t row = 0; row * 64 < S.nvec; row++) {
    const uint32_t v = row * 64 + lane_id();
    uint32_t m = v < S.nvec ? ln_mask16(rg_vec(S, v)) : 0u;
    const uint32_t c = __popc(m), inc = wave_incl_sum(c);
    const uint32_t in_row = (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
    if (rem > in_row) { rem -= in_row; continue; }
    const uint64_t reach = __ballot(inc >= rem);
    if (lane_id() == (int)__builtin_ctzll(reach)) {
      for (uint32_t j = rem - (inc - c); j > 1; j--) m &= m - 1;
      ans[q] = g.off + (S.base + 16ull * v + __builtin_ctz(m) - g.src) + 1;
    }
    return;
  }
  if (lane_id() == 0) ans[q] = ~0ull;
}

// One wave per question: the scanned count of p's tile + the newlines of that tile in front of p (the tile read only up to p).
__global__ __launch_bounds__(256) void ln_rank(const LnBlk* __restrict__ blks, const uint32_t* __restrict__ cnt, const LnAsk* __restrict__ asks, uint32_t nask,
                                               uint64_t* __restrict__ ans) {
  const uint32_t q = blockIdx.x * 4 + wave_id();
  if (q >= nask) return;
  const LnAsk A = asks[q];
  const LnBlk g = blks[A.blk];
  const uint32_t p = min(A.arg, g.len), tile = min(p / LN_TILE, ln_tiles(g.len) - 1), within = p - tile * LN_TILE;
  const LnSpan S = rg_span(g.src + (uint64_t)tile * LN_TILE, within);
  uint32_t c = 0;
  for (uint32_t v = lane_id(); v < S.nvec; v += 64) c += ln_count16(rg_vec(S, v));
  const uint32_t s = wave_sum(c);
  if (lane_id() == 0) ans[q] = (uint64_t)cnt[g.tile0 + tile] + s;
}

int bz_lines_make(const cjs_bz_index* ix, const uint32_t* counts, size_t count, cjs_bz_lines** lines) {
  *lines = nullptr;
  if (count != ix->e.size()) { set_detail("the line table is of another index"); return CJS_E_INVALID_ARG; }
  for (size_t b = 0; b < count; b++)
    if (counts[b] > ix->e[b].size) { set_detail("line table: block %zu has more newlines than bytes", b); return CJS_E_INVALID_ARG; }
  cjs_bz_lines* t = new cjs_bz_lines;
  t->nl.assign(counts, counts + count);
  t->cum.assign(count + 1, 0);
  for (size_t b = 0; b < count; b++) t->cum[b + 1] = t->cum[b] + counts[b];
  t->total_bytes = ix->off.back(); t->crc_fold = bz_lines_fold(ix);
  *lines = t;
  return 0;
}

bool lines_belong(const cjs_bz_index* ix, const cjs_bz_lines* t) {
  if (t->nl.size() == ix->e.size() && t->total_bytes == ix->off.back() && t->crc_fold == bz_lines_fold(ix)) return true;
  set_detail("the line table is of another index");
  return false;
}

}  // namespace cjs

// ---------------------------------------------------------------- the driver
namespace {

const char LN_MAGIC[8] = {'C', 'J', 'S', 'B', 'Z', 'L', 'N', '1'};
constexpr uint32_t LN_VERSION = 1;
const char* const LN_MODE[3] = {"build", "locate", "number"};
enum { LN_BUILD = 0, LN_LOCATE = 1, LN_NUMBER = 2 };

void put_le(uint8_t* p, uint64_t v, int bytes) { for (int i = 0; i < bytes; i++) p[i] = (uint8_t)(v >> (8 * i)); }
uint64_t get_le(const uint8_t* p, int bytes) { uint64_t v = 0; for (int i = 0; i < bytes; i++) v |= (uint64_t)p[i] << (8 * i); return v; }

struct LnWant { uint32_t block, arg; size_t k; };          // question k wants `arg` of index block `block`

// One call: the questions sorted by block (a batch gets its own), the counts and the answers as they come back.
struct LinesCall {
  const cjs_bz_index* ix = nullptr;
  int mode = LN_BUILD;
  std::vector<LnWant> wants; size_t want_at = 0;                   // those in front of want_at belong to earlier blocks
  std::vector<uint32_t> got;                                       // per block of the index: the newlines counted in it
  std::vector<uint64_t> ans;                                       // per question
  uint64_t h2d = 0, d2h = 0, tiles = 0;

  int batch(const RangeBatch& B) {
    std::vector<LnBlk> blks; std::vector<uint32_t> which; std::vector<LnAsk> asks; std::vector<size_t> ask_k;
    uint64_t nt = 0;
    for (size_t k = B.g0; k < B.g1; k++) {
      const uint32_t b = B.blk[k];
      while (want_at < wants.size() && wants[want_at].block < b) want_at++;
      const uint32_t len = ix->e[b].size;
      if (!B.V.good(b) || !len) continue;
      for (; want_at < wants.size() && wants[want_at].block == b; want_at++) {
        asks.push_back(LnAsk{(uint32_t)blks.size(), wants[want_at].arg}); ask_k.push_back(wants[want_at].k);
      }
      blks.push_back(LnBlk{B.addr(k), ix->off[b], len, (uint32_t)nt});
      which.push_back(b);
      nt += ln_tiles(len);
    }
    if (blks.empty()) return 0;
    if (nt > 0x7FFFFFFFull) return CJS_E_UNSUPPORTED;
    const size_t nblk = blks.size(), nask = asks.size();
    auto pad = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t o_blk = 0, o_cnt = o_blk + pad(sizeof(LnBlk) * nblk), o_tot = o_cnt + pad(4 * (size_t)nt), o_ask = o_tot + pad(4 * nblk),
                 o_ans = o_ask + pad(sizeof(LnAsk) * nask), bytes = o_ans + pad(8 * nask);
    DevBuf mem(bytes);
    if (!mem.p) return CJS_E_OUT_OF_MEMORY;
    uint8_t* d = (uint8_t*)mem.p;
    LnBlk* d_blk = (LnBlk*)(d + o_blk); uint32_t* d_cnt = (uint32_t*)(d + o_cnt); uint32_t* d_tot = (uint32_t*)(d + o_tot);
    LnAsk* d_ask = (LnAsk*)(d + o_ask); uint64_t* d_ans = (uint64_t*)(d + o_ans);
    std::vector<uint32_t> tot(nblk); std::vector<uint64_t> a(nask);
    hipStream_t s = B.s;
    int rc = 0;
    // from here on no way out without a synchronize: the copies may still be reading or writing the vectors
    if (hipMemcpyAsync(d_blk, blks.data(), sizeof(LnBlk) * nblk, hipMemcpyHostToDevice, s) != hipSuccess ||
        (nask && hipMemcpyAsync(d_ask, asks.data(), sizeof(LnAsk) * nask, hipMemcpyHostToDevice, s) != hipSuccess)) rc = CJS_E_HIP;
    else {
      hipLaunchKernelGGL(ln_count, dim3((unsigned)nt), dim3(256), 0, s, (const LnBlk*)d_blk, (uint32_t)nblk, d_cnt);
      hipLaunchKernelGGL(ln_scan, dim3((unsigned)nblk), dim3(256), 0, s, (const LnBlk*)d_blk, d_cnt, d_tot);
      if (nask && mode == LN_LOCATE)
        hipLaunchKernelGGL(ln_select, dim3((unsigned)((nask + 3) / 4)), dim3(256), 0, s, (const LnBlk*)d_blk, (const uint32_t*)d_cnt, (const uint32_t*)d_tot,
                           (const LnAsk*)d_ask, (uint32_t)nask, d_ans);
      if (nask && mode == LN_NUMBER)
        hipLaunchKernelGGL(ln_rank, dim3((unsigned)((nask + 3) / 4)), dim3(256), 0, s, (const LnBlk*)d_blk, (const uint32_t*)d_cnt, (const LnAsk*)d_ask,
                           (uint32_t)nask, d_ans);
      if (hipGetLastError() != hipSuccess || hipMemcpyAsync(tot.data(), d_tot, 4 * nblk, hipMemcpyDeviceToHost, s) != hipSuccess ||
          (nask && hipMemcpyAsync(a.data(), d_ans, 8 * nask, hipMemcpyDeviceToHost, s) != hipSuccess)) rc = CJS_E_HIP;
    }
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = CJS_E_HIP;
    if (rc) return rc;
    h2d += sizeof(LnBlk) * nblk + sizeof(LnAsk) * nask; d2h += 4 * nblk + 8 * nask; tiles += nt;
    for (size_t i = 0; i < nblk; i++) got[which[i]] = tot[i];
    for (size_t i = 0; i < nask; i++) ans[ask_k[i]] = a[i];
    return 0;
  }
};

struct LinesRun { RangeStats st; uint64_t h2d = 0, d2h = 0, tiles = 0; };

// The touched blocks through the engine with the call as its consumer: verdicts, counts and answers.
int lines_run(const uint8_t* in, const uint8_t* d_in, const cjs_bz_index* idx, const std::vector<uint32_t>& touched, LinesCall& C, RangeVerdicts& V,
              const cjs_opts* opts, LinesRun& R) {
  CallDevice cd;
  CJS_TRY(cd.select(opts));
  if (d_in && !on_device(d_in, cd.dev)) return CJS_E_INVALID_ARG;      // (no host pointer reaches a kernel)
  C.ix = idx; C.got.assign(idx->e.size(), 0);
  CJS_TRY(range_engine(in, d_in, idx, touched, V, cd.dev, R.st, [&](const RangeBatch& B) { return C.batch(B); }));
  R.h2d = R.st.h2d + C.h2d; R.d2h = R.st.d2h + C.d2h; R.tiles = C.tiles;
  return 0;
}

void lines_debug(bool device, int mode, size_t count, size_t touched, const cjs_bz_index* idx, const LinesRun& R) {
  if (!env_debug()) return;
  fprintf(stderr, "[cjs lines] %s: %s, %zu queries, %zu of %zu blocks touched, %u passes (%u row batches, %u inverse-BWT batches), upload %llu B, %llu tiles, "
          "H2D %llu D2H %llu\n", device ? "device" : "host", LN_MODE[mode], count, touched, idx->e.size(), R.st.passes, R.st.a_batches, R.st.b_batches,
          (unsigned long long)R.st.up, (unsigned long long)R.tiles, (unsigned long long)R.h2d, (unsigned long long)R.d2h);
}

int lines_build_core(const uint8_t* in, const uint8_t* d_in, size_t n, const cjs_bz_index* idx, cjs_bz_lines** lines, const cjs_opts* opts) {
  if (!lines) return CJS_E_INVALID_ARG;
  *lines = nullptr;
  clear_detail();
  if (!idx) return CJS_E_INVALID_ARG;
  CJS_TRY(check_index_stream(in ? in : d_in, n, idx));
  const std::vector<uint32_t> touched = blocks_under(idx->off, 0, idx->off.back());
  LinesCall C; LinesRun R;
  C.mode = LN_BUILD; C.got.assign(idx->e.size(), 0);
  if (!touched.empty()) {
    RangeVerdicts V(idx);
    CJS_TRY(lines_run(in, d_in, idx, touched, C, V, opts, R));
    const BadBlocks bad = V.bad_among(touched);
    if (bad.n) { V.set_bad_detail(idx, (size_t)bad.first); return CJS_E_DATA_ERROR; }
  }
  lines_debug(d_in != nullptr, LN_BUILD, 0, touched.size(), idx, R);
  return bz_lines_make(idx, C.got.data(), C.got.size(), lines);
}

int lines_ask_core(int mode, const uint8_t* in, const uint8_t* d_in, size_t n, const cjs_bz_index* idx, const cjs_bz_lines* t, const uint64_t* q, size_t count,
                   uint64_t* out, int32_t* status, const cjs_opts* opts) {
  clear_detail();
  if (!idx || !t || (count && (!q || !out || !status))) return CJS_E_INVALID_ARG;
  CJS_TRY(check_index_stream(in ? in : d_in, n, idx));
  if (!lines_belong(idx, t)) return CJS_E_INVALID_ARG;
  LinesCall C; LinesRun R;
  C.mode = mode; C.ans.assign(count, 0);
  std::vector<uint64_t> res(count, 0); std::vector<int32_t> st(count, 0);      // (the caller's arrays are written on success only)
  std::vector<uint32_t> block_of(count, ~0u);                      // ~0: the table alone answers
  for (size_t k = 0; k < count; k++) {
    const LineRoute r = mode == LN_LOCATE ? route_locate(t->cum, t->total_bytes, q[k]) : route_number(t->cum, idx->off, q[k]);
    block_of[k] = r.block; res[k] = r.value;
    if (r.block != ~0u) C.wants.push_back(LnWant{r.block, r.arg, k});
  }
  std::stable_sort(C.wants.begin(), C.wants.end(), [](const LnWant& a, const LnWant& b) { return a.block < b.block; });
  std::vector<uint32_t> touched;
  for (const LnWant& w : C.wants) if (touched.empty() || touched.back() != w.block) touched.push_back(w.block);
  if (!touched.empty()) {
    RangeVerdicts V(idx);
    CJS_TRY(lines_run(in, d_in, idx, touched, C, V, opts, R));
    bool first = true;
    for (size_t k = 0; k < count; k++) {
      const uint32_t b = block_of[k];
      if (b == ~0u) continue;
      const bool bad = !V.good(b);
      if (!bad && C.got[b] == t->nl[b] && C.ans[k] != ~0ull) { res[k] = mode == LN_LOCATE ? C.ans[k] : t->cum[b] + C.ans[k]; continue; }
      st[k] = CJS_E_DATA_ERROR;
      if (!first) continue;
      first = false;
      if (bad) V.set_bad_detail(idx, b);
      else set_detail("line table does not match the stream at block %u", b);
    }
  }
  for (size_t k = 0; k < count; k++) { out[k] = res[k]; status[k] = st[k]; }
  lines_debug(d_in != nullptr, mode, count, touched.size(), idx, R);
  return 0;
}

}  // namespace

extern "C" int cjs_bzip2_lines_build(const uint8_t* in, size_t n, const cjs_bz_index* idx, cjs_bz_lines** lines, const cjs_opts* opts) {
  CJS_GUARD_BEGIN
  if (!in && n) return CJS_E_INVALID_ARG;
  return lines_build_core(in ? in : (const uint8_t*)"", nullptr, n, idx, lines, opts);
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

extern "C" int cjs_bzip2_lines_build_device(const uint8_t* d_in, size_t n, const cjs_bz_index* idx, cjs_bz_lines** lines, const cjs_opts* opts) {
  CJS_GUARD_BEGIN
  if (!d_in && n) return CJS_E_INVALID_ARG;
  return lines_build_core(nullptr, d_in, n, idx, lines, opts);
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

extern "C" int cjs_bzip2_lines_create(const cjs_bz_index* idx, const uint32_t* counts, size_t count, cjs_bz_lines** lines) {
  if (!idx || !lines || (!counts && count)) return CJS_E_INVALID_ARG;
  clear_detail();
  CJS_GUARD_BEGIN
  return bz_lines_make(idx, counts, count, lines);
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_INVALID_ARG)
}

extern "C" int cjs_bzip2_lines_save(const cjs_bz_lines* lines, uint8_t** bytes, size_t* nbytes) {
  if (!lines || !bytes || !nbytes) return CJS_E_INVALID_ARG;
  const size_t count = lines->nl.size(), total = BZ_LINES_HEADER + 4 * count;
  uint8_t* p = (uint8_t*)malloc(total);
  if (!p) return CJS_E_OUT_OF_MEMORY;
  memcpy(p, LN_MAGIC, 8);
  put_le(p + 8, LN_VERSION, 4);
  put_le(p + 12, 0, 4);
  put_le(p + 16, count, 8);
  put_le(p + 24, lines->total_bytes, 8);
  put_le(p + 32, lines->crc_fold, 4);
  put_le(p + 36, 0, 4);
  for (size_t k = 0; k < count; k++) put_le(p + BZ_LINES_HEADER + 4 * k, lines->nl[k], 4);
  *bytes = p; *nbytes = total;
  return 0;
}

extern "C" int cjs_bzip2_lines_load(const uint8_t* bytes, size_t nbytes, const cjs_bz_index* idx, cjs_bz_lines** lines) {
  if (!lines || !idx || (!bytes && nbytes)) return CJS_E_INVALID_ARG;
  *lines = nullptr;
  clear_detail();
  CJS_GUARD_BEGIN
  if (nbytes < BZ_LINES_HEADER || memcmp(bytes, LN_MAGIC, 8) != 0) { set_detail("not a line table: bad magic"); return CJS_E_INVALID_ARG; }
  if (get_le(bytes + 8, 4) != LN_VERSION) { set_detail("line table: unknown version"); return CJS_E_INVALID_ARG; }
  if (get_le(bytes + 12, 4) != 0) { set_detail("line table: undefined flag bits"); return CJS_E_INVALID_ARG; }
  if (get_le(bytes + 36, 4) != 0) { set_detail("line table: reserved field not zero"); return CJS_E_INVALID_ARG; }
  const uint64_t count = get_le(bytes + 16, 8);
  if (count != (nbytes - BZ_LINES_HEADER) / 4 || (nbytes - BZ_LINES_HEADER) % 4) { set_detail("line table: length does not match the block count"); return CJS_E_INVALID_ARG; }
  if (count != idx->e.size() || get_le(bytes + 24, 8) != idx->off.back() || (uint32_t)get_le(bytes + 32, 4) != bz_lines_fold(idx)) {
    set_detail("the line table is of another index");
    return CJS_E_INVALID_ARG;
  }
  std::vector<uint32_t> c((size_t)count);
  for (size_t k = 0; k < (size_t)count; k++) c[k] = (uint32_t)get_le(bytes + BZ_LINES_HEADER + 4 * k, 4);
  return bz_lines_make(idx, c.data(), c.size(), lines);
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_INVALID_ARG)
}

extern "C" int cjs_bzip2_lines_info(const cjs_bz_lines* lines, uint64_t* blocks, uint64_t* newlines, uint64_t* total_bytes) {
  if (!lines) return CJS_E_INVALID_ARG;
  if (blocks) *blocks = lines->nl.size();
  if (newlines) *newlines = lines->cum.back();
  if (total_bytes) *total_bytes = lines->total_bytes;
  return 0;
}

extern "C" long cjs_bzip2_lines_counts(const cjs_bz_lines* lines, uint32_t* counts, long cap) {
  if (!lines || (!counts && cap > 0)) return CJS_E_INVALID_ARG;
  const size_t m = std::min<size_t>(lines->nl.size(), cap > 0 ? (size_t)cap : 0);
  if (m) memcpy(counts, lines->nl.data(), 4 * m);
  return (long)lines->nl.size();
}

extern "C" void cjs_bzip2_lines_destroy(cjs_bz_lines* lines) { delete lines; }

extern "C" int cjs_bzip2_lines_locate(const uint8_t* in, size_t n, const cjs_bz_index* idx, const cjs_bz_lines* lines, const uint64_t* line, size_t count,
                                      uint64_t* start, int32_t* status, const cjs_opts* opts) {
  CJS_GUARD_BEGIN
  if (!in && n) return CJS_E_INVALID_ARG;
  return lines_ask_core(LN_LOCATE, in ? in : (const uint8_t*)"", nullptr, n, idx, lines, line, count, start, status, opts);
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

extern "C" int cjs_bzip2_lines_locate_device(const uint8_t* d_in, size_t n, const cjs_bz_index* idx, const cjs_bz_lines* lines, const uint64_t* line, size_t count,
                                             uint64_t* start, int32_t* status, const cjs_opts* opts) {
  CJS_GUARD_BEGIN
  if (!d_in && n) return CJS_E_INVALID_ARG;
  return lines_ask_core(LN_LOCATE, nullptr, d_in, n, idx, lines, line, count, start, status, opts);
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

extern "C" int cjs_bzip2_lines_number(const uint8_t* in, size_t n, const cjs_bz_index* idx, const cjs_bz_lines* lines, const uint64_t* off, size_t count,
                                      uint64_t* line, int32_t* status, const cjs_opts* opts) {
  CJS_GUARD_BEGIN
  if (!in && n) return CJS_E_INVALID_ARG;
  return lines_ask_core(LN_NUMBER, in ? in : (const uint8_t*)"", nullptr, n, idx, lines, off, count, line, status, opts);
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

extern "C" int cjs_bzip2_lines_number_device(const uint8_t* d_in, size_t n, const cjs_bz_index* idx, const cjs_bz_lines* lines, const uint64_t* off, size_t count,
                                             uint64_t* line, int32_t* status, const cjs_opts* opts) {
  CJS_GUARD_BEGIN
  if (!d_in && n) return CJS_E_INVALID_ARG;
  return lines_ask_core(LN_NUMBER, nullptr, d_in, n, idx, lines, off, count, line, status, opts);
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}
