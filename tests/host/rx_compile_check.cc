// rx_compile_check.cc — the pattern compiler of the regex search (csrc/rx_compile.h) against a matcher written here: a few thousand
// random patterns from a small grammar are printed as text, compiled, and walked over random texts (rx_scan, the walk of the
// kernels); the matcher tries every way a pattern's tree can consume the text and knows nothing of automata.  Then, on patterns
// built for it: every refusal with its code and a detail that names pattern and byte, max_len and the state counts, the class map,
// the 256-byte clamp, and for every blob made that nothing in it points outside it.  Stand-alone: built with the host compiler
// under the address / undefined-behaviour sanitizers and run by tests/test_regex_compile_host.py.  Exit 0 = all checks passed.
#include "rx_compile.h"
#include <stdio.h>
#include <set>
#include <string>
#include <vector>

using namespace cjs;

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_fail < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } g_fail++; } } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }

// ---------------------------------------------------------------- the model
struct Node {
  int kind = 0;                      // 0: a byte test, 1: concatenation, 2: alternation, 3: repeat
  bool in[256] = {false}, neg = false;
  std::vector<Node> kid;
  int lo = 0, hi = 0;                // repeat: hi < 0 = no upper bound
  std::string text;                  // as the pattern spells it
};

static bool takes(const Node& n, uint8_t c, bool nocase) {
  bool hit = n.in[c];
  if (nocase && ((c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z'))) hit = hit || n.in[c ^ 32];
  return hit != n.neg;
}
// every position a match of n that starts at pos can end at
static std::set<size_t> ends(const Node& n, const std::string& t, size_t pos, bool nocase) {
  std::set<size_t> r;
  if (n.kind == 0) { if (pos < t.size() && takes(n, (uint8_t)t[pos], nocase)) r.insert(pos + 1); return r; }
  if (n.kind == 2) { for (const Node& k : n.kid) { const auto e = ends(k, t, pos, nocase); r.insert(e.begin(), e.end()); } return r; }
  if (n.kind == 1) {
    r.insert(pos);
    for (const Node& k : n.kid) { std::set<size_t> nx; for (size_t p : r) { const auto e = ends(k, t, p, nocase); nx.insert(e.begin(), e.end()); } r.swap(nx); }
    return r;
  }
  std::set<size_t> cur; cur.insert(pos);
  if (n.lo == 0) r.insert(pos);
  const int most = n.hi < 0 ? n.lo + (int)t.size() + 1 : n.hi;
  for (int c = 1; c <= most && !cur.empty(); c++) {
    std::set<size_t> nx;
    for (size_t p : cur) { const auto e = ends(n.kid[0], t, p, nocase); nx.insert(e.begin(), e.end()); }
    if (c >= n.lo) r.insert(nx.begin(), nx.end());
    cur.swap(nx);
  }
  return r;
}

// ---------------------------------------------------------------- the grammar
static const char ALPHA[] = {'a', 'b', 'B', 'c', '\n'};
static Node byte_test() {
  Node n;
  switch (rnd() % 8) {
    case 0: n.text = "."; n.in[10] = true; n.neg = true; break;
    case 1: n.text = "\\n"; n.in[10] = true; break;
    case 2: {                                                    // a class of one to three members, one of them perhaps a range
      n.neg = rnd() % 3 == 0;
      n.text = n.neg ? "[^" : "[";
      for (int k = 1 + rnd() % 3; k; k--) {
        if (rnd() % 4 == 0) { n.text += "a-c"; for (int c = 'a'; c <= 'c'; c++) n.in[c] = true; }
        else if (rnd() % 5 == 0) { n.text += "\\n"; n.in[10] = true; }
        else { const char c = ALPHA[rnd() % 4]; n.text += c; n.in[(uint8_t)c] = true; }
      }
      n.text += "]";
      break;
    }
    case 3: n.text = "\\x62"; n.in['b'] = true; break;
    default: { const char c = ALPHA[rnd() % 4]; n.text = std::string(1, c); n.in[(uint8_t)c] = true; }
  }
  return n;
}
static Node expr(int depth);
static Node repeat(int depth) {
  Node a = (depth > 0 && rnd() % 3 == 0) ? expr(depth - 1) : byte_test();
  if (a.kind != 0) a.text = (rnd() % 2 ? "(" : "(?:") + a.text + ")";
  if (rnd() % 5 < 3) return a;
  Node r; r.kind = 3;
  char buf[32];
  switch (rnd() % 7) {
    case 0: r.lo = 0; r.hi = 1; r.text = a.text + "?"; break;
    case 1: r.lo = 0; r.hi = -1; r.text = a.text + "*"; break;
    case 2: r.lo = 1; r.hi = -1; r.text = a.text + "+"; break;
    case 3: r.lo = r.hi = 1 + rnd() % 3; snprintf(buf, sizeof buf, "{%d}", r.lo); r.text = a.text + buf; break;
    case 4: r.lo = rnd() % 3; r.hi = -1; snprintf(buf, sizeof buf, "{%d,}", r.lo); r.text = a.text + buf; break;
    case 5: r.lo = 0; r.hi = 1 + rnd() % 3; snprintf(buf, sizeof buf, "{,%d}", r.hi); r.text = a.text + buf; break;
    default: r.lo = rnd() % 3; r.hi = r.lo + rnd() % 3; if (!r.hi) r.hi = 1; snprintf(buf, sizeof buf, "{%d,%d}", r.lo, r.hi); r.text = a.text + buf; break;
  }
  r.kid.push_back(a);
  return r;
}
static Node expr(int depth) {
  Node alt; alt.kind = 2;
  for (int na = rnd() % 4 == 0 ? 2 + rnd() % 2 : 1; na; na--) {
    Node cat; cat.kind = 1;
    for (int nc = 1 + rnd() % 3; nc; nc--) { cat.kid.push_back(repeat(depth)); cat.text += cat.kid.back().text; }
    alt.text += (alt.kid.empty() ? "" : "|") + cat.text;
    alt.kid.push_back(cat);
  }
  return alt;
}

// ---------------------------------------------------------------- helpers
struct Compiled { int rc; RxProgram prog; RxError err; };
static Compiled compile(const std::vector<std::string>& pats, uint32_t flags) {
  std::string all; std::vector<uint32_t> off(1, 0);
  for (const std::string& p : pats) { all += p; off.push_back((uint32_t)all.size()); }
  Compiled c;
  c.rc = rx_compile((const uint8_t*)all.data(), off.data(), (uint32_t)pats.size(), flags, c.prog, c.err);
  return c;
}
// nothing in the blob points outside it
static void check_blob(const RxProgram& R, const char* what) {
  const uint8_t* B = R.blob.data();
  RxHeader H; memcpy(&H, B, sizeof H);
  CHECK(H.nbytes <= R.blob.size() && R.blob.size() <= RX_MAX_BLOB && R.blob.size() % 16 == 0 && H.nbytes > RX_PAT, "%s: %u bytes in a blob of %zu", what, H.nbytes, R.blob.size());
  CHECK(H.npat >= 1 && H.npat <= 64 && H.nclass >= 1 && H.nclass <= 256 && H.maxlen <= 256 && H.maxlen == R.maxlen, "%s: header", what);
  for (int b = 0; b < 256; b++) {
    CHECK(B[RX_CLS + b] < H.nclass, "%s: class of byte %d", what, b);
    uint64_t m; memcpy(&m, B + RX_FIRST + 8 * b, 8);
    CHECK(H.npat == 64 || !(m >> H.npat), "%s: first[%d] names a pattern that is not there", what, b);
  }
  uint32_t end = RX_PAT + 8 * H.npat;
  for (uint32_t j = 0; j < H.npat; j++) {
    RxPat P; memcpy(&P, B + RX_PAT + 8 * j, 8);
    CHECK(P.off >= end && P.off % 4 == 0 && P.rows >= 2 && P.rows <= 257 && P.start >= 1 && P.start < P.rows, "%s: pattern %u: off %u rows %u start %u", what, j, P.off, P.rows, P.start);
    end = P.off + 2u * P.rows * H.nclass;
    CHECK(end <= H.nbytes, "%s: pattern %u's table ends at %u of %u", what, j, end, H.nbytes);
    if (end > H.nbytes) return;
    for (uint32_t k = 0; k < (uint32_t)P.rows * H.nclass; k++) {
      uint16_t e; memcpy(&e, B + P.off + 2 * k, 2);
      CHECK((e & 0xFF) < P.rows && (e >> 8) <= 1 && (k >= H.nclass || e == 0), "%s: pattern %u entry %u = %x", what, j, k, e);
    }
    CHECK(R.states[j] == (uint32_t)P.rows - 1 && R.max_len[j] <= R.maxlen, "%s: pattern %u: states and max_len", what, j);
  }
}
struct Hit { uint64_t o; uint32_t j, len; bool operator==(const Hit& x) const { return o == x.o && j == x.j && len == x.len; } };
static std::vector<Hit> scan(const RxProgram& R, const std::string& t) {
  std::vector<Hit> v;
  rx_scan(R, (const uint8_t*)t.data(), t.size(), [&](uint64_t o, uint32_t j, uint32_t len) { v.push_back(Hit{o, j, len}); });
  return v;
}

// ---------------------------------------------------------------- random patterns against the model
static void random_cases() {
  int compiled = 0, empties = 0, hits = 0, big = 0;
  for (int it = 0; it < 3000; it++) {
    const bool nocase = rnd() % 3 == 0;
    std::vector<Node> nodes;
    std::vector<std::string> pats;
    for (int np = rnd() % 4 == 0 ? 2 + rnd() % 3 : 1; np; np--) { nodes.push_back(expr(2)); pats.push_back(nodes.back().text); }
    bool empty = false;
    for (const Node& n : nodes) empty = empty || ends(n, "", 0, nocase).count(0);
    Compiled c = compile(pats, nocase ? CJS_SEARCH_NOCASE : 0);
    if (c.rc == CJS_E_UNSUPPORTED && strstr(c.err.text, "states")) { big++; continue; }      // (it may stand in front of an empty one)
    if (empty) { empties++; CHECK(c.rc == CJS_E_INVALID_ARG && strstr(c.err.text, "empty"), "%s: a pattern that matches the empty string gave %d", pats[0].c_str(), c.rc); continue; }
    CHECK(c.rc == 0, "%s (and %zu more): %d %s", pats[0].c_str(), pats.size() - 1, c.rc, c.err.text);
    if (c.rc) continue;
    compiled++;
    check_blob(c.prog, pats[0].c_str());
    for (int tx = 0; tx < 3; tx++) {
      std::string t;
      for (int n = 1 + rnd() % 30; n; n--) t += ALPHA[rnd() % 5];
      std::vector<Hit> want;
      for (size_t o = 0; o < t.size(); o++)
        for (size_t j = 0; j < nodes.size(); j++) {
          const auto e = ends(nodes[j], t, o, nocase);
          if (!e.empty() && *e.rbegin() > o) want.push_back(Hit{o, (uint32_t)j, (uint32_t)(*e.rbegin() - o)});
        }
      const std::vector<Hit> got = scan(c.prog, t);
      hits += (int)want.size();
      CHECK(got == want, "pattern %s%s (of %zu) on a text of %zu bytes: %zu matches, the matcher finds %zu", pats[0].c_str(), nocase ? " (nocase)" : "", pats.size(), t.size(), got.size(),
            want.size());
      for (size_t j = 0; j < nodes.size(); j++) for (const Hit& h : want) if (h.j == j) CHECK(h.len <= c.prog.max_len[j], "%s: a match longer than max_len", pats[j].c_str());
    }
  }
  CHECK(compiled > 1500 && empties > 50 && hits > 5000 && big < 100, "the grammar: %d compiled, %d empty, %d too big, %d matches", compiled, empties, big, hits);
}

// ---------------------------------------------------------------- patterns built for it
static void refusal(const std::vector<std::string>& pats, int code, int pattern, int pos, const char* word) {
  const Compiled c = compile(pats, 0);
  CHECK(c.rc == code && c.err.code == code, "%s: %d, expected %d (%s)", pats.back().c_str(), c.rc, code, c.err.text);
  char head[64];
  snprintf(head, sizeof head, "pattern %d, byte %d: ", pattern, pos);
  CHECK(strncmp(c.err.text, head, strlen(head)) == 0 && strstr(c.err.text, word), "%s: the detail is '%s', expected '%s...%s'", pats.back().c_str(), c.err.text, head, word);
}
static void refusals() {
  const int INV = CJS_E_INVALID_ARG, UNS = CJS_E_UNSUPPORTED;
  refusal({"^a"}, UNS, 0, 0, "anchor");
  refusal({"a$"}, UNS, 0, 1, "anchor");
  refusal({"ok", "\\bfoo"}, UNS, 1, 0, "escaped letter");
  refusal({"x\\Bfoo"}, UNS, 0, 1, "escaped letter");
  refusal({"\\Afoo"}, UNS, 0, 0, "escaped letter");
  refusal({"foo\\Z"}, UNS, 0, 3, "escaped letter");
  refusal({"\\q"}, UNS, 0, 0, "escaped letter");
  refusal({"(a)\\1"}, UNS, 0, 3, "backreference");
  refusal({"a*?"}, UNS, 0, 2, "lazy");
  refusal({"a++"}, UNS, 0, 2, "possessive");
  refusal({"a{2}?"}, UNS, 0, 4, "lazy");
  refusal({"(?=a)b"}, UNS, 0, 0, "(?:");
  refusal({"(?P<n>a)"}, UNS, 0, 0, "(?:");
  refusal({"(?i)a"}, UNS, 0, 0, "(?:");
  refusal({"b(?<!a)"}, UNS, 0, 1, "(?:");
  refusal({"a*"}, INV, 0, 0, "empty");
  refusal({"x", "y", "(a|)"}, INV, 2, 0, "empty");
  refusal({"()"}, INV, 0, 0, "empty");
  refusal({"a{0}"}, INV, 0, 0, "empty");
  refusal({"("}, INV, 0, 0, "unbalanced (");
  refusal({"a(b(c)"}, INV, 0, 1, "unbalanced (");
  refusal({"a)"}, INV, 0, 1, "unbalanced )");
  refusal({"[a"}, INV, 0, 0, "unbalanced [");
  refusal({"x[]"}, INV, 0, 1, "unbalanced [");
  refusal({"[z-a]"}, INV, 0, 1, "backwards");
  refusal({"[a-\\d]"}, INV, 0, 1, "range");
  refusal({"*a"}, INV, 0, 0, "nothing to repeat");
  refusal({"a|+"}, INV, 0, 2, "nothing to repeat");
  refusal({"(?:?)"}, INV, 0, 3, "nothing to repeat");
  refusal({"a**"}, INV, 0, 2, "behind a quantifier");
  refusal({"a{2}{3}"}, INV, 0, 4, "behind a quantifier");
  refusal({"a{3,2}"}, INV, 0, 1, "n < m");
  refusal({"a{257}"}, INV, 0, 1, "above 256");
  refusal({"a{1,257}"}, INV, 0, 1, "above 256");
  refusal({"a{x}"}, INV, 0, 1, "malformed");
  refusal({"a{2"}, INV, 0, 1, "malformed");
  refusal({"\\x4"}, INV, 0, 0, "\\x");
  refusal({"a\\xg0"}, INV, 0, 1, "\\x");
  refusal({"a\\"}, INV, 0, 1, "at the end");
  refusal({"a", ""}, INV, 1, 0, "1..1024");
  refusal({std::string(1025, 'a')}, INV, 0, 0, "1..1024");
  refusal(std::vector<std::string>(65, "a"), INV, 0, 0, "1 to 64");
  refusal({}, INV, 0, 0, "1 to 64");
  refusal({"(a|b)*a(a|b){8}"}, UNS, 0, 0, "255 states");
  refusal({"(x{200}){3}"}, UNS, 0, 0, "255 states");
  refusal({"((((a{256}){256}){256}){256}){256}"}, UNS, 0, 0, "255 states");
  refusal({"(a|b)*a(a|b){40}"}, UNS, 0, 0, "255 states");
  refusal(std::vector<std::string>(64, "[a-z]{200}"), UNS, 37, 0, "32768 bytes");
  Compiled c = compile({"a"}, 2);
  CHECK(c.rc == INV && strstr(c.err.text, "flag"), "undefined flag bits: %d", c.rc);
  const uint32_t bad_off[3] = {1, 2, 3};
  CHECK(rx_compile((const uint8_t*)"abcd", bad_off, 2, 0, c.prog, c.err) == INV && strstr(c.err.text, "pat_off[0]"), "pat_off[0] != 0");
}

static void one(const char* pat, uint32_t flags, uint32_t states, uint32_t max_len, uint32_t nclass) {
  const Compiled c = compile({pat}, flags);
  CHECK(c.rc == 0, "%s: %d %s", pat, c.rc, c.err.text);
  if (c.rc) return;
  check_blob(c.prog, pat);
  RxHeader H; memcpy(&H, c.prog.blob.data(), sizeof H);
  CHECK(c.prog.states[0] == states && c.prog.max_len[0] == max_len && H.nclass == nclass, "%s: %u states, max_len %u, %u classes; expected %u, %u, %u", pat, c.prog.states[0],
        c.prog.max_len[0], H.nclass, states, max_len, nclass);
}
static void counts() {
  one("a", 0, 1, 1, 2);                        // the start row alone: its one live entry accepts and leads nowhere
  one("abc", 0, 3, 3, 4);
  one("a+", 0, 1, 256, 2);                     // the start state is the loop
  one("ab|cd", 0, 3, 2, 5);
  one("a{2,5}", 0, 5, 5, 2);
  one("[ab]|a", 0, 1, 1, 2);                   // a and b act alike: one class
  one("[Z-a]", CJS_SEARCH_NOCASE, 1, 1, 2);
  one("a.*b", 0, 2, 256, 4);                   // a, b, newline, the rest
  one("x{256}", 0, 256, 256, 2);
  one("\\xF7[^\\xF7]{254,}", 0, 255, 256, 2);      // the 254th byte's state is the loop
  one("b[ab]{0,255}", 0, 256, 256, 3);
  one("\\xF7\\xF7[^\\xF7]{254}", 0, 256, 256, 2);
  one("\\xF7+[^\\xF7]{1,255}", 0, 256, 256, 2);
  one("(a|b)*a(a|b){7}", 0, 128, 256, 3);     // the last seven bytes are the state; the eighth back decides on the step
  one("[a-z]{200}", 0, 200, 200, 2);
  one("(ab|c)[^a]{1,3}\\.", 0, 6, 6, 5);
  one("\\d{2}-\\d", 0, 4, 4, 3);
  one("[^\\x00-\\xff]", 0, 1, 0, 1);           // nothing matches it
}

static void clamp_and_case() {
  Compiled c = compile({"x{256}"}, 0);
  std::vector<Hit> got = scan(c.prog, std::string(300, 'x'));
  CHECK(got.size() == 45 && got[0] == (Hit{0, 0, 256}) && got[44] == (Hit{44, 0, 256}), "x{256} on 300 x: %zu matches", got.size());
  c = compile({"x+"}, 0);
  got = scan(c.prog, std::string(300, 'x'));
  CHECK(got.size() == 300 && got[0].len == 256 && got[44].len == 256 && got[45].len == 255 && got[299].len == 1, "x+ on 300 x: the clamp at 256 and at the end");
  c = compile({"\\xF7[^\\xF7]{254,}"}, 0);
  got = scan(c.prog, "\xF7" + std::string(254, 'q') + "\xF7" + std::string(400, 'q'));
  CHECK(got.size() == 2 && got[0] == (Hit{0, 0, 255}) && got[1] == (Hit{255, 0, 256}), "255 bytes up to the next 0xF7, 256 of the 401 behind it: %zu matches", got.size());
  c = compile({"a.*b"}, 0);
  got = scan(c.prog, "a--b-b\nb a" + std::string(300, '-') + "b");
  CHECK(got.size() == 1 && got[0] == (Hit{0, 0, 6}), "a.*b stops at the newline and sees no b 301 bytes away");
  c = compile({"[^A-C]{2}9", "[Z-a]", "\xC1"}, CJS_SEARCH_NOCASE);
  got = scan(c.prog, "bd9xB9dd9[`\xE1\xC1zA");
  const std::vector<Hit> want = {{6, 0, 3}, {9, 1, 1}, {10, 1, 1}, {12, 2, 1}, {13, 1, 1}, {14, 1, 1}};
  CHECK(got == want, "nocase classes: %zu matches", got.size());
  c = compile(std::vector<std::string>(64, "ab"), 0);
  got = scan(c.prog, "xab");
  CHECK(c.rc == 0 && got.size() == 64 && got[63] == (Hit{1, 63, 2}), "64 patterns at one offset");
}

int main() {
  random_cases();
  refusals();
  counts();
  clamp_and_case();
  if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
  printf("rx_compile_check ok\n");
  return 0;
}
