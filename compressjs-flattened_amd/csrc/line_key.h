// line_key.h -- the arithmetic of a line's key (cjs_bz_linekey) as linekeys.hip computes it in pieces.  No HIP: the
// kernels and the host compiler read the same functions (tests/host/line_key_check.cc checks them against naive 128-bit
// arithmetic).
//   P = 2^61 - 1.  The bases B1, B2 = 256 + (s mod (P - 256)), s the first and the second output of splitmix64 started at `seed`.
//   For bytes b_0 .. b_{m-1}:  H_B = sum (b_i + 1) * B^(m-1-i) mod P; the empty string gives 0.  (b + 1, so that a zero byte
//   moves the hash: "\0", "\0\0" and "" differ in the hash and not only in the length.)
//   key = { H_B1, low 32 bits of m, low 32 bits of H_B2 }.
// H is linear in the string: H(A|B) = H(A) * B^|B| + H(B).  A FRAGMENT carries both hashes in full and its length, so two of them
// join into the fragment of their concatenation; a line that spans tiles, blocks, batches or passes is the join of its pieces.
// The bases are PUBLIC for a given seed: whoever knows the seed can make two different lines of one key.  A caller who faces
// crafted input passes a seed of its own.  Equal keys mean equal lines only up to a collision: about 61 + 32 = 93 bits of hash,
// plus the length.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "cjs_hip.h"

#if defined(__HIPCC__)
#define LK_FN __host__ __device__ __forceinline__
#else
#define LK_FN inline
#endif

namespace cjs {

constexpr uint64_t LK_P = (1ull << 61) - 1;

// x < 2^62 -> x mod P
LK_FN uint64_t lk_fold(uint64_t x) {
  x = (x & LK_P) + (x >> 61);
  return x >= LK_P ? x - LK_P : x;
}
// a * b mod P for a, b < 2^61: with a * b = hi * 2^64 + lo and 2^61 = 1 (mod P) it is (hi * 8 + lo / 2^61) + (lo mod 2^61)
LK_FN uint64_t lk_mul(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint64_t lo = a * b, hi = __umul64hi(a, b);
#else
  const unsigned __int128 p = (unsigned __int128)a * b;
  const uint64_t lo = (uint64_t)p, hi = (uint64_t)(p >> 64);
#endif
  return lk_fold(((hi << 3) | (lo >> 61)) + (lo & LK_P));      // (hi < 2^58: both terms are below 2^61)
}
LK_FN uint64_t lk_add(uint64_t a, uint64_t b) { const uint64_t s = a + b; return s >= LK_P ? s - LK_P : s; }      // a, b < P
// B^n by squaring
LK_FN uint64_t lk_pow(uint64_t base, uint64_t n) {
  uint64_t r = 1;
  while (n) {
    if (n & 1) r = lk_mul(r, base);
    base = lk_mul(base, base);
    n >>= 1;
  }
  return r;
}

struct LkBases { uint64_t b1, b2; };
LK_FN uint64_t lk_splitmix(uint64_t& state) {
  uint64_t z = (state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
LK_FN LkBases lk_bases(uint64_t seed) {
  LkBases B;
  B.b1 = 256 + lk_splitmix(seed) % (LK_P - 256);
  B.b2 = 256 + lk_splitmix(seed) % (LK_P - 256);
  return B;
}

// A fragment: both hashes of `len` bytes.  The empty one is {0, 0, 0}.
struct LkFrag { uint64_t h1, h2, len; };
// the fragment with byte c behind it: one Horner step of either hash
LK_FN void lk_push(LkFrag& f, const LkBases& B, uint8_t c) {
  f.h1 = lk_add(lk_mul(f.h1, B.b1), (uint64_t)c + 1);
  f.h2 = lk_add(lk_mul(f.h2, B.b2), (uint64_t)c + 1);
  f.len++;
}
// a | b when p1 = B1^b.len and p2 = B2^b.len are at hand, and when they are not
LK_FN LkFrag lk_join_pw(const LkFrag& a, const LkFrag& b, uint64_t p1, uint64_t p2) {
  LkFrag r;
  r.h1 = lk_add(lk_mul(a.h1, p1), b.h1);
  r.h2 = lk_add(lk_mul(a.h2, p2), b.h2);
  r.len = a.len + b.len;
  return r;
}
LK_FN LkFrag lk_join(const LkFrag& a, const LkFrag& b, const LkBases& B) {
  if (a.len == 0) return b;
  return lk_join_pw(a, b, lk_pow(B.b1, b.len), lk_pow(B.b2, b.len));
}
LK_FN cjs_bz_linekey lk_key(const LkFrag& f) {
  cjs_bz_linekey k;
  k.hash = f.h1; k.len = (uint32_t)f.len; k.check = (uint32_t)f.h2;
  return k;
}
// "this line touches a bad block": no key of a line, whose hash is below P
LK_FN cjs_bz_linekey lk_bad_key() {
  cjs_bz_linekey k;
  k.hash = ~0ull; k.len = ~0u; k.check = ~0u;
  return k;
}
LK_FN bool lk_is_bad(const cjs_bz_linekey& k) { return k.hash == ~0ull && k.len == ~0u && k.check == ~0u; }
// two lines are taken as equal iff their records are; the bad record equals nothing, itself included
LK_FN bool lk_same(const cjs_bz_linekey& a, const cjs_bz_linekey& b) {
  return a.hash == b.hash && a.len == b.len && a.check == b.check && !lk_is_bad(a);
}

// The keys of the lines of text[0 .. n): one per newline and one for the unterminated tail (which may be empty).  keys gets the
// first min(cap, lines) of them; returns the number of lines.
inline size_t lk_text_keys(const uint8_t* text, size_t n, uint64_t seed, cjs_bz_linekey* keys, size_t cap) {
  const LkBases B = lk_bases(seed);
  LkFrag f{0, 0, 0};
  size_t lines = 0;
  for (size_t i = 0; i < n; i++) {
    lk_push(f, B, text[i]);
    if (text[i] != 0x0A) continue;
    if (lines < cap) keys[lines] = lk_key(f);
    lines++;
    f = LkFrag{0, 0, 0};
  }
  if (lines < cap) keys[lines] = lk_key(f);
  return lines + 1;
}

}  // namespace cjs
