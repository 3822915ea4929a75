// rx_compile.h -- the pattern compiler of the bounded regular-expression search (regex.hip) and the walk its
// kernels and cjs_stage_regex_scan share.  Pattern text -> byte-set AST -> Thompson NFA -> subset construction -> a minimised
// machine per pattern, all of a call laid out as one blob that the kernels copy into LDS.  No HIP in here
// (tests/host/rx_compile_check.cc compiles it with the host compiler).
//
// The machine is anchored: it is walked from one start position over at most 256 bytes and remembers the last step that accepted.
// Acceptance stands on the TRANSITION, not on the state: an entry says where a (state, class) pair leads and whether the bytes up
// to and including this one are a match.  A state that accepts and leads nowhere is then the dead state, and the start state, which
// most patterns never enter again, needs no byte value of its own: `x{256}` has 256 rows behind the dead one and fits the 8-bit
// entry.  Minimisation is Moore's partition refinement on these outputs; whatever cannot reach an accepting transition falls into
// the dead state's block, so a walk stops at the first byte that rules a match out.
//
// The blob (little-endian; offsets in bytes):
//   0     RxHeader   npat, nclass, maxlen (the longest possible match of any pattern, <= 256), nbytes (the blob's size)
//   16    cls[256]   byte -> class: the coarsest partition of the bytes that every pattern's table respects
//   272   first[256] 64-bit masks: bit j = byte b does not kill pattern j's start state (it leads on, or it is a match by itself)
//   2320  RxPat[npat] off (of the pattern's table), start (its start row), rows
//   ...   the tables: rows x nclass entries of 16 bits, row 0 the dead state; low byte = the next state, high byte = 1 if this
//         step accepts.  One 16-bit LDS read per byte of a walk answers both questions.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <map>
#include <vector>
#include "cjs_hip.h"

#if defined(__HIPCC__)
#define RX_FN __host__ __device__ __forceinline__
#else
#define RX_FN inline
#endif

namespace cjs {

constexpr uint32_t RX_MAXP = CJS_SEARCH_MAX_PATTERNS, RX_MAXL = CJS_SEARCH_MAX_PATTERN_BYTES;
constexpr uint32_t RX_MAX_TEXT = CJS_REGEX_MAX_PATTERN_TEXT;      // bytes of a pattern's text
constexpr uint32_t RX_MAX_BOUND = 256;           // of {m,n}
constexpr uint32_t RX_MAX_STATES = 255;          // states a transition enters: the values of an entry's low byte besides 0
constexpr uint32_t RX_MAX_NFA = 1u << 13, RX_MAX_DFA = 1024;      // what the construction may grow to before it gives up (a bound on its host time)
constexpr uint32_t RX_MAX_BLOB = CJS_REGEX_MAX_TABLE_BYTES;

struct RxHeader { uint32_t npat, nclass, maxlen, nbytes; };
struct RxPat { uint32_t off; uint16_t start, rows; };
constexpr uint32_t RX_CLS = sizeof(RxHeader), RX_FIRST = RX_CLS + 256, RX_PAT = RX_FIRST + 256 * 8;
static_assert(RX_FIRST % 8 == 0 && sizeof(RxPat) == 8, "first[] is read as 64-bit words");

RX_FN uint64_t rx_first(const uint8_t* blob, uint8_t b) { return reinterpret_cast<const uint64_t*>(blob + RX_FIRST)[b]; }

// The longest match of pattern j among the prefixes of t[0 .. room), room <= 256; 0: none.  The walk ends in the dead state.
RX_FN uint32_t rx_walk(const uint8_t* blob, uint32_t j, const uint8_t* t, uint32_t room) {
  const uint32_t ncls = reinterpret_cast<const RxHeader*>(blob)->nclass;
  const RxPat P = reinterpret_cast<const RxPat*>(blob + RX_PAT)[j];
  const uint16_t* tab = reinterpret_cast<const uint16_t*>(blob + P.off);
  const uint8_t* cls = blob + RX_CLS;
  uint32_t s = P.start, best = 0;
  for (uint32_t k = 0; k < room; k++) {
    const uint32_t e = tab[s * ncls + cls[t[k]]];
    if (e >> 8) best = k + 1;
    s = e & 0xFFu;
    if (!s) break;
  }
  return best;
}

// ---------------------------------------------------------------- sets and the AST
struct RxSet {
  uint64_t w[4] = {0, 0, 0, 0};
  void add(uint32_t b) { w[b >> 6] |= 1ull << (b & 63); }
  void add(uint32_t lo, uint32_t hi) { for (uint32_t b = lo; b <= hi; b++) add(b); }
  bool has(uint32_t b) const { return (w[b >> 6] >> (b & 63)) & 1; }
  void join(const RxSet& o) { for (int i = 0; i < 4; i++) w[i] |= o.w[i]; }
  void negate() { for (int i = 0; i < 4; i++) w[i] = ~w[i]; }
  void close_case() { for (uint32_t c = 'a'; c <= 'z'; c++) if (has(c) || has(c - 32)) { add(c); add(c - 32); } }      // 'A'..'Z' and 'a'..'z' alike
  bool operator<(const RxSet& o) const { return memcmp(w, o.w, sizeof w) < 0; }
};

struct RxError { int code = 0; uint32_t pattern = 0, pos = 0; char text[200] = {0}; };

// the refusal of pattern err.pattern at byte `at`: code and the detail text "pattern J, byte P: what"; returns the code
inline int rx_refuse(RxError& err, int code, uint32_t at, const char* what) {
  err.code = code; err.pos = at;
  snprintf(err.text, sizeof err.text, "pattern %u, byte %u: %s", err.pattern, at, what);
  return code;
}

enum { RX_SET, RX_EMPTY, RX_CAT, RX_ALT, RX_REP };
struct RxAst { int kind, a, b, lo, hi; };      // SET: a = its set; CAT, ALT: a, b; REP: a{lo,hi}, hi < 0: no upper bound

// the recursive-descent parser of one pattern; a negative return is an error, told in err
struct RxParser {
  const uint8_t* p; uint32_t n; bool nocase; std::vector<RxAst>& ast; std::vector<RxSet>& sets; RxError& err;
  uint32_t i = 0;

  int fail(int code, uint32_t at, const char* what) { rx_refuse(err, code, at, what); return -1; }
  int mk(int kind, int a = 0, int b = 0, int lo = 0, int hi = 0) { ast.push_back(RxAst{kind, a, b, lo, hi}); return (int)ast.size() - 1; }
  int mk_set(RxSet s) { if (nocase) s.close_case(); sets.push_back(s); return mk(RX_SET, (int)sets.size() - 1); }

  static bool alpha(uint8_t c) { return (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z'); }
  static bool digit(uint8_t c) { return c >= '0' && c <= '9'; }
  static int hex(uint8_t c) { return digit(c) ? c - '0' : (c >= 'a' && c <= 'f') ? c - 'a' + 10 : (c >= 'A' && c <= 'F') ? c - 'A' + 10 : -1; }

  // the escape at p[i] == '\\': a set; one = it is a single byte
  int escape(RxSet& s, bool& one) {
    const uint32_t at = i;
    if (i + 1 >= n) return fail(CJS_E_INVALID_ARG, at, "a \\ at the end");
    const uint8_t c = p[i + 1];
    i += 2; one = false;
    RxSet d; d.add('0', '9');
    RxSet w = d; w.add('a', 'z'); w.add('A', 'Z'); w.add('_');
    RxSet sp; sp.add(' '); sp.add(9, 13);
    switch (c) {
      case 'd': s = d; return 0;
      case 'w': s = w; return 0;
      case 's': s = sp; return 0;
      case 'D': s = d; s.negate(); return 0;
      case 'W': s = w; s.negate(); return 0;
      case 'S': s = sp; s.negate(); return 0;
    }
    one = true;
    switch (c) {
      case 'n': s.add(10); return 0;
      case 'r': s.add(13); return 0;
      case 't': s.add(9); return 0;
      case 'f': s.add(12); return 0;
      case 'v': s.add(11); return 0;
      case 'x': {
        if (i + 2 > n || hex(p[i]) < 0 || hex(p[i + 1]) < 0) return fail(CJS_E_INVALID_ARG, at, "\\x needs two hexadecimal digits");
        s.add((uint32_t)(hex(p[i]) * 16 + hex(p[i + 1]))); i += 2;
        return 0;
      }
    }
    if (digit(c)) return fail(CJS_E_UNSUPPORTED, at, "backreferences and octal escapes are not supported");
    if (alpha(c)) return fail(CJS_E_UNSUPPORTED, at, "this escaped letter is not supported (anchors and word boundaries need the byte in front of a match)");
    s.add(c);
    return 0;
  }

  int bracket() {
    const uint32_t open = i++;
    bool neg = false, first = true;
    if (i < n && p[i] == '^') { neg = true; i++; }
    RxSet all;
    for (;; first = false) {
      if (i >= n) return fail(CJS_E_INVALID_ARG, open, "unbalanced [");
      if (p[i] == ']' && !first) { i++; break; }
      const uint32_t at = i;
      RxSet s; bool one = true;
      if (p[i] == '\\') { if (escape(s, one) < 0) return -1; }
      else s.add(p[i++]);
      if (i + 1 < n && p[i] == '-' && p[i + 1] != ']') {
        if (!one) return fail(CJS_E_INVALID_ARG, at, "a class escape as the end of a range");
        i++;
        RxSet t; bool one2 = true;
        if (p[i] == '\\') { if (escape(t, one2) < 0) return -1; }
        else t.add(p[i++]);
        if (!one2) return fail(CJS_E_INVALID_ARG, at, "a class escape as the end of a range");
        uint32_t lo = 0, hi = 0;
        while (!s.has(lo)) lo++;
        while (!t.has(hi)) hi++;
        if (hi < lo) return fail(CJS_E_INVALID_ARG, at, "a range that runs backwards");
        s.add(lo, hi);
      }
      all.join(s);
    }
    if (nocase) all.close_case();
    if (neg) all.negate();
    sets.push_back(all);
    return mk(RX_SET, (int)sets.size() - 1);
  }

  // {m}, {m,}, {,n}, {m,n} at p[i] == '{'
  int bounds(int& lo, int& hi) {
    const uint32_t at = i++;
    auto number = [&](int& v) { bool any = false; v = 0; while (i < n && digit(p[i])) { v = std::min(v * 10 + (p[i++] - '0'), 100000); any = true; } return any; };
    const bool has_lo = number(lo);
    bool has_hi = false, comma = false;
    if (i < n && p[i] == ',') { comma = true; i++; has_hi = number(hi); }
    if (i >= n || p[i] != '}' || (!has_lo && !has_hi)) return fail(CJS_E_INVALID_ARG, at, "a malformed {m,n} (a literal { is written \\{)");
    i++;
    if (!comma) hi = lo;
    else if (!has_hi) hi = -1;
    if (lo > (int)RX_MAX_BOUND || hi > (int)RX_MAX_BOUND) return fail(CJS_E_INVALID_ARG, at, "a repeat bound above 256");
    if (hi >= 0 && hi < lo) return fail(CJS_E_INVALID_ARG, at, "{m,n} with n < m");
    return 0;
  }

  int atom() {
    const uint32_t at = i;
    const uint8_t c = p[i];
    switch (c) {
      case '(': {
        i++;
        if (i < n && p[i] == '?') {
          if (i + 1 < n && p[i + 1] == ':') i += 2;
          else return fail(CJS_E_UNSUPPORTED, at, "of the (?...) groups only (?:...) is supported");
        }
        const int r = alt();
        if (r < 0) return -1;
        if (i >= n || p[i] != ')') return fail(CJS_E_INVALID_ARG, at, "unbalanced (");
        i++;
        return r;
      }
      case '[': return bracket();
      case '.': { i++; RxSet s; s.add(10); s.negate(); return mk_set(s); }
      case '^': case '$': return fail(CJS_E_UNSUPPORTED, at, "anchors are not supported (a start position does not know the byte in front of it)");
      case '*': case '+': case '?': case '{': return fail(CJS_E_INVALID_ARG, at, "a quantifier with nothing to repeat");
      case '\\': { RxSet s; bool one; if (escape(s, one) < 0) return -1; return mk_set(s); }
    }
    i++;
    RxSet s; s.add(c);
    return mk_set(s);
  }

  int rep() {
    int a = atom();
    if (a < 0 || i >= n) return a;
    int lo = 0, hi = -1;
    switch (p[i]) {
      case '*': i++; break;
      case '+': lo = 1; i++; break;
      case '?': hi = 1; i++; break;
      case '{': if (bounds(lo, hi) < 0) return -1; break;
      default: return a;
    }
    if (i < n && (p[i] == '?' || p[i] == '+')) return fail(CJS_E_UNSUPPORTED, i, "lazy and possessive quantifiers are not supported");
    if (i < n && (p[i] == '*' || p[i] == '{')) return fail(CJS_E_INVALID_ARG, i, "a quantifier behind a quantifier");
    return mk(RX_REP, a, 0, lo, hi);
  }
  int cat() {
    int l = -1;
    while (i < n && p[i] != '|' && p[i] != ')') {
      const int r = rep();
      if (r < 0) return -1;
      l = l < 0 ? r : mk(RX_CAT, l, r);
    }
    return l < 0 ? mk(RX_EMPTY) : l;
  }
  int alt() {
    int l = cat();
    while (l >= 0 && i < n && p[i] == '|') {
      i++;
      const int r = cat();
      if (r < 0) return -1;
      l = mk(RX_ALT, l, r);
    }
    return l;
  }
  int parse() {
    const int r = alt();
    if (r >= 0 && i < n) return fail(CJS_E_INVALID_ARG, i, "unbalanced )");
    return r;
  }
};

// ---------------------------------------------------------------- NFA, DFA, the minimised machine
// A Thompson NFA: a node has up to two empty edges, or one edge on a set.
struct RxNfa {
  std::vector<int> e1, e2, set, to;
  bool full = false;
  int node() {
    if (e1.size() >= RX_MAX_NFA) { full = true; return 0; }
    e1.push_back(-1); e2.push_back(-1); set.push_back(-1); to.push_back(-1);
    return (int)e1.size() - 1;
  }
  struct Frag { int in, out; };      // `out` has no edge yet
  Frag emit(const std::vector<RxAst>& ast, int k) {
    const RxAst& A = ast[k];
    if (full) return Frag{0, 0};
    switch (A.kind) {
      case RX_SET: { const int s = node(), t = node(); set[s] = A.a; to[s] = t; return Frag{s, t}; }
      case RX_EMPTY: { const int s = node(); return Frag{s, s}; }
      case RX_CAT: { const Frag x = emit(ast, A.a), y = emit(ast, A.b); e1[x.out] = y.in; return Frag{x.in, y.out}; }
      case RX_ALT: {
        const Frag x = emit(ast, A.a), y = emit(ast, A.b);
        const int s = node(), t = node();
        e1[s] = x.in; e2[s] = y.in; e1[x.out] = t; e1[y.out] = t;
        return Frag{s, t};
      }
    }
    // a{lo,hi}: lo copies, then a star or hi - lo optional copies
    const int s = node();
    int out = s;
    for (int c = 0; c < A.lo && !full; c++) { const Frag x = emit(ast, A.a); e1[out] = x.in; out = x.out; }
    if (A.hi < 0) {
      const Frag x = emit(ast, A.a);
      const int t = node();
      e1[out] = x.in; e2[out] = t; e1[x.out] = x.in; e2[x.out] = t;
      out = t;
    } else {
      for (int c = A.lo; c < A.hi && !full; c++) {
        const Frag x = emit(ast, A.a);
        const int t = node();
        e1[out] = x.in; e2[out] = t; e1[x.out] = t;
        out = t;
      }
    }
    return Frag{s, out};
  }
};

// One pattern's machine over the provisional classes: ent[row * ncls + c] = next | accept << 8, row 0 dead.
struct RxMachine { std::vector<uint16_t> ent; uint32_t rows = 0, start = 0, max_len = 0; };

// rep[c]: a byte of provisional class c.  0, or the error in err.
inline int rx_machine(const std::vector<RxAst>& ast, int root, const std::vector<RxSet>& sets, const std::vector<uint8_t>& rep, RxMachine& M, RxError& err) {
  const uint32_t ncls = (uint32_t)rep.size();
  RxNfa N;
  const RxNfa::Frag F = N.emit(ast, root);
  if (N.full) return rx_refuse(err, CJS_E_UNSUPPORTED, 0, "too large: more than 255 states");
  // subset construction; state 0 = the empty set
  std::vector<uint32_t> stamp(N.e1.size(), 0);
  uint32_t tick = 0;
  std::vector<int> stack;
  auto closure = [&](std::vector<int>& v) {
    tick++;
    stack.assign(v.begin(), v.end());
    v.clear();
    for (int x : stack) stamp[x] = tick;
    while (!stack.empty()) {
      const int x = stack.back(); stack.pop_back();
      v.push_back(x);
      for (int y : {N.e1[x], N.e2[x]}) if (y >= 0 && stamp[y] != tick) { stamp[y] = tick; stack.push_back(y); }
    }
    std::sort(v.begin(), v.end());
  };
  std::map<std::vector<int>, uint32_t> ids;
  std::vector<std::vector<int>> dstate(1);
  std::vector<uint8_t> acc(1, 0);
  std::vector<uint32_t> trans(ncls, 0);
  ids[dstate[0]] = 0;
  auto intern = [&](std::vector<int>& v) {
    auto it = ids.find(v);
    if (it != ids.end()) return it->second;
    const uint32_t id = (uint32_t)dstate.size();
    ids[v] = id; dstate.push_back(v);
    acc.push_back(std::binary_search(v.begin(), v.end(), F.out));
    trans.resize(trans.size() + ncls, 0);
    return id;
  };
  std::vector<int> v(1, F.in);
  closure(v);
  const uint32_t d_start = intern(v);
  if (acc[d_start]) return rx_refuse(err, CJS_E_INVALID_ARG, 0, "the pattern matches the empty string");
  for (uint32_t d = 1; d < dstate.size(); d++) {
    const std::vector<int> from = dstate[d];                         // (a copy: intern() grows dstate)
    for (uint32_t c = 0; c < ncls; c++) {
      v.clear();
      for (int x : from) if (N.set[x] >= 0 && sets[N.set[x]].has(rep[c])) v.push_back(N.to[x]);
      if (v.empty()) continue;
      std::sort(v.begin(), v.end()); v.erase(std::unique(v.begin(), v.end()), v.end());
      closure(v);
      const uint32_t t = intern(v);
      trans[d * ncls + c] = t;
      if (dstate.size() > RX_MAX_DFA) return rx_refuse(err, CJS_E_UNSUPPORTED, 0, "too large: more than 255 states");
    }
  }
  // Moore's refinement on the outputs of the transitions: block[d], the dead state's block numbered 0
  const uint32_t nd = (uint32_t)dstate.size();
  std::vector<uint32_t> block(nd, 0), sig;
  uint32_t nblocks = 0;
  for (bool outputs = true;; outputs = false) {
    std::map<std::vector<uint32_t>, uint32_t> seen;
    std::vector<uint32_t> nb(nd);
    for (uint32_t d = 0; d < nd; d++) {
      sig.assign(1, outputs ? 0 : block[d]);
      for (uint32_t c = 0; c < ncls; c++) sig.push_back(outputs ? acc[trans[d * ncls + c]] : block[trans[d * ncls + c]]);
      nb[d] = seen.emplace(sig, (uint32_t)seen.size()).first->second;      // (state 0 comes first: its block is 0)
    }
    block.swap(nb);
    if (!outputs && seen.size() == nblocks) break;
    nblocks = (uint32_t)seen.size();
  }
  // the blocks a transition enters get the values 1 .. T in breadth-first order; the start block one of them, or the row behind
  std::vector<uint32_t> member(nblocks, 0), num(nblocks, 0), order;
  for (uint32_t d = 0; d < nd; d++) member[block[d]] = d;
  std::vector<uint8_t> reached(nblocks, 0), entered(nblocks, 0);
  std::vector<uint32_t> bfs(1, block[d_start]);
  reached[bfs[0]] = 1;
  for (size_t q = 0; q < bfs.size(); q++)
    for (uint32_t c = 0; c < ncls; c++) {
      const uint32_t t = block[trans[member[bfs[q]] * ncls + c]];
      if (!t) continue;
      if (!entered[t]) { entered[t] = 1; order.push_back(t); }
      if (!reached[t]) { reached[t] = 1; bfs.push_back(t); }
    }
  if (order.size() > RX_MAX_STATES) return rx_refuse(err, CJS_E_UNSUPPORTED, 0, "more than 255 states");
  for (size_t k = 0; k < order.size(); k++) num[order[k]] = (uint32_t)k + 1;
  const uint32_t sb = block[d_start];
  if (!entered[sb]) { num[sb] = (uint32_t)order.size() + 1; order.push_back(sb); }
  M.start = num[sb]; M.rows = (uint32_t)order.size() + 1;
  M.ent.assign((size_t)M.rows * ncls, 0);
  for (uint32_t b : order)
    for (uint32_t c = 0; c < ncls; c++) {
      const uint32_t t = trans[member[b] * ncls + c];
      M.ent[(size_t)num[b] * ncls + c] = (uint16_t)(num[block[t]] | (acc[t] ? 0x100u : 0u));
    }
  // the longest match, up to 256: the last step at which some path accepts
  std::vector<uint8_t> cur(M.rows, 0), nxt;
  cur[M.start] = 1; M.max_len = 0;
  for (uint32_t k = 1; k <= RX_MAXL; k++) {
    nxt.assign(M.rows, 0);
    bool any = false;
    for (uint32_t s = 1; s < M.rows; s++) if (cur[s])
      for (uint32_t c = 0; c < ncls; c++) {
        const uint16_t e = M.ent[(size_t)s * ncls + c];
        if (e >> 8) M.max_len = k;
        if (e & 0xFF) { nxt[e & 0xFF] = 1; any = true; }
      }
    if (!any) break;
    cur.swap(nxt);
  }
  return 0;
}

// ---------------------------------------------------------------- a call's patterns
struct RxProgram {
  std::vector<uint8_t> blob;                       // (padded with zeros to a multiple of 16 bytes; header.nbytes is the size that counts)
  uint32_t maxlen = 1;                             // the longest possible match of any pattern, 1..256
  std::vector<uint32_t> states, max_len;           // per pattern: rows besides the dead one; the longest possible match
};

// Pattern j = pat[pat_off[j] .. pat_off[j+1]).  0, or CJS_E_INVALID_ARG / CJS_E_UNSUPPORTED with err filled in.
inline int rx_compile(const uint8_t* pat, const uint32_t* pat_off, uint32_t npat, uint32_t flags, RxProgram& out, RxError& err) {
  auto refuse = [&](int code, uint32_t j, const char* what) { err.pattern = j; return rx_refuse(err, code, 0, what); };
  if (npat < 1 || npat > RX_MAXP) return refuse(CJS_E_INVALID_ARG, 0, "1 to 64 patterns");
  if (flags & ~(uint32_t)CJS_SEARCH_NOCASE) return refuse(CJS_E_INVALID_ARG, 0, "undefined flag bits");
  if (pat_off[0] != 0) return refuse(CJS_E_INVALID_ARG, 0, "pat_off[0] is not 0");
  for (uint32_t j = 0; j < npat; j++)
    if (pat_off[j + 1] <= pat_off[j] || pat_off[j + 1] - pat_off[j] > RX_MAX_TEXT) return refuse(CJS_E_INVALID_ARG, j, "a pattern text outside 1..1024 bytes");
  std::vector<RxSet> sets;
  std::vector<std::vector<RxAst>> asts(npat);
  std::vector<int> roots(npat);
  for (uint32_t j = 0; j < npat; j++) {
    err.pattern = j;
    RxParser P{pat + pat_off[j], pat_off[j + 1] - pat_off[j], (flags & CJS_SEARCH_NOCASE) != 0, asts[j], sets, err};
    if ((roots[j] = P.parse()) < 0) return err.code;
  }
  // provisional classes: bytes that belong to the same sets
  std::map<std::vector<uint8_t>, uint32_t> by_sig;
  std::vector<uint8_t> pcls(256), rep;
  {
    std::vector<RxSet> uniq(sets);
    std::sort(uniq.begin(), uniq.end());
    uniq.erase(std::unique(uniq.begin(), uniq.end(), [](const RxSet& a, const RxSet& b) { return !(a < b) && !(b < a); }), uniq.end());
    for (uint32_t b = 0; b < 256; b++) {
      std::vector<uint8_t> sig((uniq.size() + 7) / 8, 0);
      for (size_t k = 0; k < uniq.size(); k++) if (uniq[k].has(b)) sig[k >> 3] |= (uint8_t)(1u << (k & 7));
      const auto it = by_sig.emplace(sig, (uint32_t)by_sig.size());
      if (it.second) rep.push_back((uint8_t)b);
      pcls[b] = (uint8_t)it.first->second;
    }
  }
  const uint32_t npc = (uint32_t)rep.size();
  std::vector<RxMachine> M(npat);
  for (uint32_t j = 0; j < npat; j++) {
    err.pattern = j;
    if (const int rc = rx_machine(asts[j], roots[j], sets, rep, M[j], err)) return rc;      // (a refusal of the whole pattern: byte 0)
  }
  // the classes: provisional ones with the same column in every table are one
  std::map<std::vector<uint16_t>, uint32_t> by_col;
  std::vector<uint32_t> final_of(npc), col_rep;
  for (uint32_t c = 0; c < npc; c++) {
    std::vector<uint16_t> col;
    for (const RxMachine& m : M) for (uint32_t s = 0; s < m.rows; s++) col.push_back(m.ent[(size_t)s * npc + c]);
    const auto it = by_col.emplace(col, (uint32_t)by_col.size());
    if (it.second) col_rep.push_back(c);
    final_of[c] = it.first->second;
  }
  const uint32_t ncls = (uint32_t)col_rep.size();
  size_t nbytes = RX_PAT + sizeof(RxPat) * npat;
  std::vector<RxPat> rec(npat);
  for (uint32_t j = 0; j < npat; j++) {
    rec[j] = RxPat{(uint32_t)nbytes, (uint16_t)M[j].start, (uint16_t)M[j].rows};
    nbytes += ((size_t)M[j].rows * ncls * 2 + 3) & ~(size_t)3;
    if (nbytes > RX_MAX_BLOB) {
      err.code = CJS_E_UNSUPPORTED; err.pattern = j; err.pos = 0;
      snprintf(err.text, sizeof err.text, "pattern %u, byte 0: the tables of patterns 0..%u take more than %u bytes", j, j, RX_MAX_BLOB);
      return CJS_E_UNSUPPORTED;
    }
  }
  out.blob.assign((nbytes + 15) & ~(size_t)15, 0);
  out.states.resize(npat); out.max_len.resize(npat); out.maxlen = 1;      // (at least 1: the halo and the carry are maxlen - 1 bytes)
  uint8_t* B = out.blob.data();
  for (uint32_t b = 0; b < 256; b++) B[RX_CLS + b] = (uint8_t)final_of[pcls[b]];
  for (uint32_t j = 0; j < npat; j++) {
    memcpy(B + RX_PAT + sizeof(RxPat) * j, &rec[j], sizeof(RxPat));
    for (uint32_t s = 0; s < M[j].rows; s++)
      for (uint32_t c = 0; c < ncls; c++) {
        const uint16_t e = M[j].ent[(size_t)s * npc + col_rep[c]];
        memcpy(B + rec[j].off + 2 * ((size_t)s * ncls + c), &e, 2);
      }
    out.states[j] = M[j].rows - 1; out.max_len[j] = M[j].max_len;
    out.maxlen = std::max(out.maxlen, M[j].max_len);
  }
  for (uint32_t b = 0; b < 256; b++) {
    uint64_t m = 0;
    for (uint32_t j = 0; j < npat; j++) if (M[j].ent[(size_t)M[j].start * npc + pcls[b]]) m |= 1ull << j;
    memcpy(B + RX_FIRST + 8 * b, &m, 8);
  }
  const RxHeader H{npat, ncls, out.maxlen, (uint32_t)nbytes};
  memcpy(B, &H, sizeof H);
  return 0;
}

// Every (o, j, L) of text[0 .. n) in (off, pattern) order, by the walk the kernels do: on(o, j, L).
template <typename F>
inline void rx_scan(const RxProgram& R, const uint8_t* text, size_t n, F on) {
  const uint8_t* B = R.blob.data();
  const uint32_t npat = reinterpret_cast<const RxHeader*>(B)->npat;
  for (size_t o = 0; o < n; o++) {
    const uint64_t m = rx_first(B, text[o]);
    const uint32_t room = (uint32_t)std::min<size_t>(n - o, R.maxlen);
    for (uint32_t j = 0; j < npat; j++) if ((m >> j) & 1) { const uint32_t len = rx_walk(B, j, text + o, room); if (len) on((uint64_t)o, j, len); }
  }
}

}  // namespace cjs
