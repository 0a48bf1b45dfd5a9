// Scalar field Fr = Z / r (r the order of G1 / G2): what the Lagrange coefficients of a threshold recovery are computed in
// (shares.cuh).  Eight little-endian 32-bit words, Montgomery form with R = 2^256; every function keeps its result in [0, r).
// The data is public (identifiers, coefficients), so the arithmetic is variable time: the inversion is a plain Fermat
// exponentiation, the final subtractions branch.
// The multiplication is CIOS with 32 x 32 -> 64-bit products (v_mad_u64_u32 on gfx950): for a < 2^256 and b < r the result is
// below 2 r before its one conditional subtraction, so fr_to_mont also takes a non-canonical 256-bit input.
// Also compiles as plain C++ for the host harness tests/hostsim_shares (fp.cuh supplies BLS_FN).
#pragma once
#include "fp.cuh"

struct fr {
  uint32_t w[8];
};

BLS_CONST uint32_t FR_MOD[8] = {0x00000001u, 0xffffffffu, 0xfffe5bfeu, 0x53bda402u, 0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u};
BLS_CONST uint32_t FR_R2[8] = {0xf3f29c6du, 0xc999e990u, 0x87925c23u, 0x2b6cedcbu, 0x7254398fu, 0x05d31496u, 0x9f59ff11u, 0x0748d9d9u};   // 2^512 mod r
BLS_CONST uint32_t FR_R3[8] = {0x439b73afu, 0xc62c1807u, 0x8cf06990u, 0x1b3e0d18u, 0xc7b5f418u, 0x73d13c71u, 0xc8db33e9u, 0x6e2a5bb9u};   // 2^768 mod r
BLS_CONST uint32_t FR_ONE_M[8] = {0xfffffffeu, 0x00000001u, 0x00034802u, 0x5884b7fau, 0xecbc4ff5u, 0x998c4fefu, 0xacc5056fu, 0x1824b159u}; // 2^256 mod r
BLS_CONST uint32_t FR_RM2[8] = {0xffffffffu, 0xfffffffeu, 0xfffe5bfeu, 0x53bda402u, 0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u}; // r - 2
#define FR_N0 0xffffffffu   // -r^-1 mod 2^32 (r = 1 mod 2^32)

// v < r as a 256-bit little-endian value (the canonical check of an identifier)
BLS_FN bool fr_words_canonical(const uint32_t v[8]) {
  for (int j = 7; j >= 0; j--) {
    if (v[j] != FR_MOD[j]) return v[j] < FR_MOD[j];
  }
  return false;   // v == r
}
BLS_FN bool fr_is_zero(const fr& a) {
  uint32_t o = 0;
  for (int j = 0; j < 8; j++) o |= a.w[j];
  return o == 0;
}
BLS_FN bool fr_eq(const fr& a, const fr& b) {
  uint32_t o = 0;
  for (int j = 0; j < 8; j++) o |= a.w[j] ^ b.w[j];
  return o == 0;
}
// r = v - r when v >= r (v given with a ninth word `hi`)
BLS_FN void fr_final_sub(fr& o, const uint32_t v[8], uint32_t hi) {
  uint32_t d[8];
  uint64_t bw = 0;
  for (int j = 0; j < 8; j++) {
    const uint64_t t = (uint64_t)v[j] - FR_MOD[j] - bw;
    d[j] = (uint32_t)t;
    bw = (t >> 63) & 1;
  }
  const bool ge = hi || !bw;
  for (int j = 0; j < 8; j++) o.w[j] = ge ? d[j] : v[j];
}
// o = a b / 2^256 mod r  (a < 2^256, b < r)
BLS_FN void fr_mul(fr& o, const fr& a, const fr& b) {
  uint32_t t[10];
  for (int j = 0; j < 10; j++) t[j] = 0;
  for (int i = 0; i < 8; i++) {
    uint64_t c = 0;
    for (int j = 0; j < 8; j++) {
      const uint64_t s = (uint64_t)a.w[j] * b.w[i] + t[j] + c;
      t[j] = (uint32_t)s;
      c = s >> 32;
    }
    uint64_t s = (uint64_t)t[8] + c;
    t[8] = (uint32_t)s;
    t[9] = (uint32_t)(s >> 32);
    const uint32_t m = t[0] * FR_N0;
    s = (uint64_t)m * FR_MOD[0] + t[0];
    c = s >> 32;
    for (int j = 1; j < 8; j++) {
      s = (uint64_t)m * FR_MOD[j] + t[j] + c;
      t[j - 1] = (uint32_t)s;
      c = s >> 32;
    }
    s = (uint64_t)t[8] + c;
    t[7] = (uint32_t)s;
    t[8] = t[9] + (uint32_t)(s >> 32);
  }
  fr_final_sub(o, t, t[8]);
}
BLS_FN void fr_sub(fr& o, const fr& a, const fr& b) {
  uint32_t d[8];
  uint64_t bw = 0;
  for (int j = 0; j < 8; j++) {
    const uint64_t t = (uint64_t)a.w[j] - b.w[j] - bw;
    d[j] = (uint32_t)t;
    bw = (t >> 63) & 1;
  }
  if (bw) {
    uint64_t c = 0;
    for (int j = 0; j < 8; j++) {
      const uint64_t t = (uint64_t)d[j] + FR_MOD[j] + c;
      d[j] = (uint32_t)t;
      c = t >> 32;
    }
  }
  for (int j = 0; j < 8; j++) o.w[j] = d[j];
}
BLS_FN void fr_add(fr& o, const fr& a, const fr& b) {
  uint32_t s[8];
  uint64_t c = 0;
  for (int j = 0; j < 8; j++) {
    const uint64_t t = (uint64_t)a.w[j] + b.w[j] + c;
    s[j] = (uint32_t)t;
    c = t >> 32;
  }
  fr_final_sub(o, s, (uint32_t)c);
}
BLS_FN void fr_one(fr& o) {
  for (int j = 0; j < 8; j++) o.w[j] = FR_ONE_M[j];
}
// any 256-bit value -> Montgomery form of (v mod r)
BLS_FN void fr_to_mont(fr& o, const uint32_t v[8]) {
  fr a, r2;
  for (int j = 0; j < 8; j++) {
    a.w[j] = v[j];
    r2.w[j] = FR_R2[j];
  }
  fr_mul(o, a, r2);
}
// a 512-bit little-endian value (sixteen words) -> Montgomery form of (v mod r): Scalar::from_bytes_wide.  With lo and hi the two
// halves, v R = lo R + hi 2^256 R, and one Montgomery product each gives lo R^2 / R and hi R^3 / R.
BLS_FN void fr_from_wide(fr& o, const uint32_t v[16]) {
  fr lo, hi, r2, r3;
  for (int j = 0; j < 8; j++) {
    lo.w[j] = v[j];
    hi.w[j] = v[8 + j];
    r2.w[j] = FR_R2[j];
    r3.w[j] = FR_R3[j];
  }
  fr_mul(lo, lo, r2);
  fr_mul(hi, hi, r3);
  fr_add(o, lo, hi);
}
// Montgomery form -> the canonical value in [0, r)
BLS_FN void fr_from_mont(uint32_t v[8], const fr& a) {
  fr one, t;
  for (int j = 0; j < 8; j++) one.w[j] = j == 0 ? 1u : 0u;
  fr_mul(t, a, one);
  for (int j = 0; j < 8; j++) v[j] = t.w[j];
}
// a^(r - 2) (Fermat; 0 -> 0), left-to-right square and multiply over the 255 bits of r - 2
BLS_FN void fr_inv(fr& o, const fr& a) {
  fr acc;
  fr_one(acc);
  for (int bit = 254; bit >= 0; bit--) {
    fr_mul(acc, acc, acc);
    if ((FR_RM2[bit >> 5] >> (bit & 31)) & 1u) fr_mul(acc, acc, a);
  }
  o = acc;
}
